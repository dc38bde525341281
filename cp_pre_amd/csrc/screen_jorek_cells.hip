// screen_jorek_cells.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) against PER-CELL sets for the reduced-MHD (JOREK) residuals (libcp_pre_screenjorekcells.so,
// include/cp_pre_screenjorekcells.h): per sample, max |r| / m and the number of cells with |r| <= q_k[cell] * m[cell] at up to
// 16 levels, in the launch that evaluates r.  The residual is never written.
//
// Nothing new runs on the device: this is the cell <Form, Single, CellSets> of screen_entries.h's table that screen_cells.hip
// leaves out for JOREK.  The marches are screen_march.h's and screen_flat.h's with their per-cell sets policy (CellSets,
// screen_plane.h: the level quads, the end of a plane and the block order told at the head of screen_cells.hip), the functors
// star_march.h's JorekContinuity / JorekTemperature, which take the radius R as one more field of which only the centre value
// is read.  The host side is screen_entries.h's body jorek and its jorek_views, as in screen_jorek.hip, so the checks, their
// order and the return codes are that body's; this object's flags are star_march.o's (csrc/Makefile), so the residual in
// registers is the one pre_residual_jorek_f32 would have stored.
//
// What this unit adds is the batch size below: how many level quads a thread holds ACROSS the functor (CellsBatch); the
// quads beyond them are fetched after it, the same number at a time (CellsLate's default, screen_plane.h).  Every tap
// structure of both equations is built in both forms and none has scratch (resources.sh screen_jorek_cells.hip; DESIGN 4.29
// has the figures): nothing here needs a row in the table Built.
#include "screen_march.h"
#include "screen_flat.h"
#include "../../include/cp_pre_screenjorekcells.h"
#include "screen_entries.h"

// The batch size and its measurement variant (csrc/Makefile: SCREENJOREKCELLS_BATCH).  All 16 level quads fit both marches
// without scratch in every tap structure (continuity 154-186 registers, temperature 176-222: two or three waves per SIMD); in
// batches of 4 the functors take 105-146 and 128-176 (a third or fourth wave).  Measured on the layout the scripts hold
// (Nt-fastest [96,3,256,256,40], the reference's tap structure, nk = 10): batches of 4 take 1.57 ms for the
// temperature equation and 1.45 ms for the continuity equation, all 16 across the functor 2.13 and 2.02 ms - so 4 is the
// default for both functors.  (4 across the functor and the other 12 in ONE batch after it measured 1.55 and 1.41 ms, 2-3 %
// less; that takes a late batch size of this unit's own, which screen_cells_pair.hip alone states: not built here.)  The
// other tap structures and the Ny-fastest march take the same size and have not been timed apart.
#ifndef PRE_SCREENJOREKCELLS_BATCH
#define PRE_SCREENJOREKCELLS_BATCH 4
#endif
static_assert(PRE_SCREENJOREKCELLS_BATCH >= 1 && PRE_SCREENJOREKCELLS_BATCH <= NKMAX && NKMAX % PRE_SCREENJOREKCELLS_BATCH == 0,
              "whole batches of 1 to 16 level quads");

namespace {

template <int M> struct CellsBatch<JorekContinuity<M>, void> { static constexpr int value = PRE_SCREENJOREKCELLS_BATCH; };
template <int M> struct CellsBatch<JorekTemperature<M>, void> { static constexpr int value = PRE_SCREENJOREKCELLS_BATCH; };

}  // namespace

extern "C" {

int pre_screenjorekcells_abi_version(void) { return PRE_SCREENJOREKCELLS_ABI_VERSION; }
int pre_screenjorekcells_sample_group(void) { return CELLS_G; }

int pre_screenjorekcells_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                             const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                             const float coef[4], const pre_screencells_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb) return PRE_E_NULL;
    return jorek<NyForm, Single, CellSets>(eq, jorek_views(eq, fields, Rb), K_t, K_R, K_Z, K_RR, K_ZZ, coef, s, B, T, X, Y, flags,
                                           stream);
}

int pre_screenjorekcells_flat_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                                  const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                                  const float coef[4], const pre_screencellsflat_t *s,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb) return PRE_E_NULL;
    return jorek<FlatForm, Single, CellSets>(eq, jorek_views(eq, fields, Rb), K_t, K_R, K_Z, K_RR, K_ZZ, coef, s, B, T, X, Y, flags,
                                             stream);
}

}  // extern "C"
