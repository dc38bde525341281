// screen_cells_pair.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) against PER-CELL sets for the data-driven scores d = r(a) - r(b) of two field sets (libcp_pre_screencellspair.so,
// include/cp_pre_screencellspair.h): per sample, max |d| / m and the number of cells with |d| <= q_k[cell] * m[cell] at up to
// 16 levels, in the launch that evaluates both residuals.  Neither residual nor their difference is written.
//
// Nothing new runs on the device: this is the one cell <Form, Paired, CellSets> of screen_entries.h's table that
// screen_pair.hip (<Form, Paired, ScalarSets>) and screen_cells.hip (<Form, Single, CellSets>) leave out.  The marches are
// screen_march.h's and screen_flat.h's with their per-cell sets policy (CellSets, screen_plane.h: the level quads, the end of
// a plane and the block order told at the head of screen_cells.hip), the functor is Paired<Fn> (paired_functor.h) over
// star_march.h's Linear1, Linear2, NSMomentum and MHDContinuity, each half rounded to fp32 before the subtraction.  The host
// side of an entry is screen_entries.h's: the entry hands the 2F views of both sets (pair_views) to the body of its kind, so
// every check of host_checks.h is made of every view of both sets and the level strides go through prepare_sets; this
// object's flags are star_march.o's (csrc/Makefile), so each half in registers is the residual the single-set pass would
// have stored.
//
// What this unit adds is the batch sizes below.  A paired functor holds two neighbourhoods; what it leaves of the 256
// registers decides how many level quads a thread can hold ACROSS it (CellsBatch).  After it the neighbourhoods are dead and
// the rest of the levels come in batches of CellsLate, which screen_plane.h sizes apart from the first: the paired NS
// momentum has room for one quad across its evaluation and for fifteen after it, two waits per plane whatever nk.
//
// Built: Paired<Linear1>, Paired<Linear2>, Paired<MHDContinuity<M>> in the reference's tap structure and the y-fixed one
// (M = 0, 1 Ny-fastest; 3, 4 Nt-fastest) and Paired<NSMomentum<M>> in the reference's (M = 0; 3).  The y-fixed paired NS
// momentum and the general stars are not built (the table Built of screen_entries.h, with the figures): their entry returns
// PRE_E_UNSUPPORTED.  No instantiation that is built has scratch (resources.sh screen_cells_pair.hip).
#include "screen_march.h"
#include "screen_flat.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screencellspair.h"
#include "screen_entries.h"

// measurement variants (csrc/Makefile: SCREENCELLSPAIR_BATCH, SCREENCELLSPAIR_LATE): caps on the two batch sizes
#ifndef PRE_SCREENCELLSPAIR_BATCH
#define PRE_SCREENCELLSPAIR_BATCH 16
#endif
#ifndef PRE_SCREENCELLSPAIR_LATE
#define PRE_SCREENCELLSPAIR_LATE 16
#endif
static_assert(PRE_SCREENCELLSPAIR_BATCH >= 1 && PRE_SCREENCELLSPAIR_BATCH <= NKMAX, "a first batch of 1 to 16 level quads");
static_assert(PRE_SCREENCELLSPAIR_LATE >= 1 && PRE_SCREENCELLSPAIR_LATE <= NKMAX, "later batches of 1 to 16 level quads");

namespace {

// PairRoom<Fn>: the level quads Paired<Fn> holds across its evaluation.  At most what fits both marches without scratch
// (resources.sh screen_cells_pair.hip: every instantiation built has spill 0, scratch 0): with 16, Paired<Linear2> has 8 bytes
// of scratch on the merged-row march, the y-fixed paired MHD continuity 28-32 / 8 bytes, and the paired NS momentum 240-244 /
// 148 bytes (84 / 20 with 8, 8 on the tiled march with 2: it fits with one).  Paired<Linear1> has room for all 16 but is
// measured faster with 4 and the other 12 after it (113-123 registers in place of 162-172: a fourth wave per SIMD; 4.4
// against 6.7 ms on two [512,32,256,256] sets, Ny-fastest, 4.7 against 7.3 ms Nt-fastest: DESIGN 4.28).
template <class Fn> struct PairRoom { static constexpr int value = NKMAX; };
template <> struct PairRoom<Linear1> { static constexpr int value = 4; };
template <> struct PairRoom<Linear2> { static constexpr int value = 8; };
template <> struct PairRoom<MHDContinuity<1>> { static constexpr int value = 8; };
template <> struct PairRoom<MHDContinuity<4>> { static constexpr int value = 8; };
template <int M> struct PairRoom<NSMomentum<M>> { static constexpr int value = 1; };

// the later batches: the rest of the levels at once, or the widest whole share of it the cap allows
constexpr int late_batch(int first)
{
    if (first == NKMAX) return NKMAX;                // (no later batch)
    int n = NKMAX - first;
    if (n > PRE_SCREENCELLSPAIR_LATE) n = PRE_SCREENCELLSPAIR_LATE;
    while ((NKMAX - first) % n != 0) --n;
    return n;
}

template <class Fn> struct CellsBatch<Paired<Fn>, void> {
    static constexpr int value = PairRoom<Fn>::value < PRE_SCREENCELLSPAIR_BATCH ? PairRoom<Fn>::value : PRE_SCREENCELLSPAIR_BATCH;
};
template <class Fn> struct CellsLate<Paired<Fn>, void> { static constexpr int value = late_batch(CellsBatch<Paired<Fn>>::value); };

}  // namespace

extern "C" {

int pre_screencellspair_abi_version(void) { return PRE_SCREENCELLSPAIR_ABI_VERSION; }
int pre_screencellspair_sample_group(void) { return CELLS_G; }

// ---------------------------------------------------------------- Ny-fastest fields: screen_march.h
int pre_screencellspair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off,
                                      int ntaps, const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                      void *stream)
{
    return stencil3d<NyForm, Paired, CellSets>({{a, b}, 2}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screencellspair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                    float ratio, const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                    void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return linear2<NyForm, Paired, CellSets>(pair_views<2>(a, b), K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screencellspair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                        const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                        const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                        void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return ns_momentum<NyForm, Paired, CellSets>(pair_views<3>(a, b), K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y,
                                                 flags, stream);
}

int pre_screencellspair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                           const float *K_y, double gamma, const pre_screencells_t *s, int64_t B, int64_t T,
                                           int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return mhd<NyForm, Paired, CellSets>(0, pair_views<3>(a, b), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

// ---------------------------------------------------------------- Nt-fastest fields: screen_flat.h
int pre_screencellspair_flat_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off,
                                           int ntaps, const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y,
                                           int flags, void *stream)
{
    return stencil3d<FlatForm, Paired, CellSets>({{a, b}, 2}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screencellspair_flat_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                         float ratio, const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y,
                                         int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return linear2<FlatForm, Paired, CellSets>(pair_views<2>(a, b), K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screencellspair_flat_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                             const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                             const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                             void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return ns_momentum<FlatForm, Paired, CellSets>(pair_views<3>(a, b), K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y,
                                                   flags, stream);
}

int pre_screencellspair_flat_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                                const float *K_y, double gamma, const pre_screencellsflat_t *s, int64_t B,
                                                int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return mhd<FlatForm, Paired, CellSets>(0, pair_views<3>(a, b), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
