"""Import-path shim: ``from Utils.ConvOps_0d import ConvOperator`` (Inverse_residuals/DHO/DHO_NODE.py:25)."""
from cp_pre_amd.convops_0d import ConvOperator, get_stencil  # noqa: F401
