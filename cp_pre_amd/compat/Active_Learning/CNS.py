"""Import-path shim: ``from Active_Learning.CNS import Euler_FV_OS_rhs`` (Active_Learning/CNS.py:6-38).

The reference file's second class, ``CNS_residuals`` (:42), is left out: its ``mass`` method reads ``self.rho``, which no
line of the class defines, so it cannot run in the reference either."""
from cp_pre_amd.cns import Euler_FV_OS_rhs  # noqa: F401
