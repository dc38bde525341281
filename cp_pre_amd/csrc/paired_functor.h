// paired_functor.h - Paired<Fn>: a residual functor evaluated on two field sets, stated once for pair_march.hip
// (libcp_pre_pair.so: the difference is stored) and screen_pair.hip (libcp_pre_screenpair.so: the difference is screened).
#pragma once
#include "star_march.h"

namespace {

// A functor of 2*Fn::F views: views [0, F) are the truth set, [F, 2F) the prediction set, and
// eval = Fn::eval(first half) - Fn::eval(second half).
template <class Fn>
struct Paired {
    static constexpr int F = 2 * Fn::F;
    static_assert(F <= MAXF, "a paired functor must fit the march's field views");
    // (no cap: the paired NS momentum in the Nt-fastest relabelling, the heaviest, needs more than the 128 VGPRs its
    // single-set twin is capped at, and spilling in the plane loop cost 30 % once - NSMomentum)
    static constexpr int MIN_WAVES = 1;
    static constexpr unsigned XMASK = XMask<Fn>::value | (XMask<Fn>::value << Fn::F);
    using Params = typename Fn::Params;
    static __device__ __forceinline__ float4 eval(const Nbr (&n)[F], const Params &p)
    {
        // each half rounded to fp32 before the difference, as numpy subtracts the two residual arrays
        const float4 a = Fn::eval(*reinterpret_cast<const Nbr(*)[Fn::F]>(&n[0]), p);
        const float4 b = Fn::eval(*reinterpret_cast<const Nbr(*)[Fn::F]>(&n[Fn::F]), p);
        return a - b;
    }
};

template <int M> using PairedNS = Paired<NSMomentum<M>>;
template <int M> using PairedMHDContinuity = Paired<MHDContinuity<M>>;

}  // namespace
