/* cp_pre_dist.h - C ABI of libcp_pre_dist.so: the device sweeps of the sharded marginal calibration by histogram
 * exchange (cp_pre_amd.pipeline.marginal_qhat(..., exchange="histogram")).
 *
 * The per-cell q-hat over all n_local x W samples of a batch sharded over W ranks (Marginal/MHD_Residuals_CP.py:388-418,
 * Marginal/NS_Residuals_CP.py:307-337: one np.quantile over the whole batch) without moving every score to the rank
 * that owns its cell: the ranks agree on each cell's value window, reduce per-cell bucket histograms, and send only
 * the scores that fall in a bucket holding a wanted rank.  The collectives are the caller's (torch.distributed); this
 * library holds the four passes over device memory.
 *
 * Scores are addressed like pre_kth_axis0_planes_f32 (cp_pre_hip.h): `planes` score matrices [n, per], plane p at
 * scores + p*plane_stride, its rows row_stride apart.  Cell g (0 <= g < planes*per) is cell g % per of plane g / per.
 * A RUN is the cells [c0, c0 + C); it is padded to Cp = W*Co cells, rank r owning cells [r*Co, (r+1)*Co) of it.
 * Keys are the order-preserving uint32 image of fp32 (ascending floats <-> ascending uints).
 *
 * Every call is asynchronous on the given HIP stream; no global atomics, no workspace: each workgroup owns the whole
 * column of 64 adjacent cells, so every result is bitwise reproducible.
 * Return codes: 0 ok; < 0 as in cp_pre_hip.h (PRE_E_*); > 0 a hipError_t.  Every refusal is returned before any launch
 * and writes nothing:
 *   PRE_E_NULL   a null pointer (scores, an output, a table; only `send` and `vals` may be null, when nothing is sent or
 *                received), or a source or run that cannot be addressed: n, per, planes, W or Co <= 0, C or c0 < 0,
 *                C > W*Co, c0 + C > planes*per, row_stride < per with n > 1, plane_stride < per with planes > 1,
 *                W > 65535 or more than 2^31 - 1 tiles; for the pick W > 64*1024 or Co <= 0;
 *   PRE_E_RANGE  S or nk outside [1, PRE_DIST_MAX_SLOTS], packed != 0 with n*W > 32767, the pick's Co > 2^31 - 1.
 */
#ifndef CP_PRE_DIST_H
#define CP_PRE_DIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_DIST_ABI_VERSION 1
#define PRE_DIST_NB 256          /* buckets per cell */
#define PRE_DIST_PICK_CAP 2048   /* longest candidate list (all ranks' segments of one cell and slot) the pick holds */
#define PRE_DIST_MAX_SLOTS 64    /* slots (distinct wanted buckets) per cell; also the most ranks per call */

int pre_dist_abi_version(void);

/* win [3, Cp] int32, for every cell c < Cp of the run (MIN-reducible across ranks):
 *   win[0][c] = (int32)(klo ^ 0x80000000),  klo = least key over the cell's non-NaN scores;
 *   win[1][c] = (int32)(~khi ^ 0x80000000), khi = greatest key over them   (no non-NaN score: the MIN identities);
 *   win[2][c] = 0 if the cell holds a NaN, else 1.
 * Pad cells (C <= c < Cp) read nothing and are written as a NaN-free constant 0.0. */
int pre_dist_window_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n, int64_t per,
                        int64_t c0, int64_t C, int64_t W, int64_t Co, int32_t *win, void *stream);

/* params [3, Cp] int32 (the caller derives them from the group's window): params[0][c] = klo, params[1][c] = the bits of
 * the fp32 scale sf > 0 of the value-linear map, or 0 for the key-linear one, params[2][c] = its shift s, or < 0: the
 * cell takes no part (NaN, constant or pad).  bucket(v) = max(0, min(NB-1, (int)((v - key2f(klo)) * sf))) (fp32, no
 * contraction, truncated) when sf > 0, else min(NB-1, (key(v) - klo) >> s) in uint32 arithmetic.  Both forms are clamped
 * at both ends so that no score can index outside the NB counters; inside the window only the upper clamp of the
 * value-linear form ever binds (at the window's top).  A score outside the agreed window [klo, khi] is the caller's
 * error: it is counted in an end bucket, and the two forms do not agree on which (a key below klo wraps to NB-1 in
 * the key-linear form and clamps to 0 in the value-linear one), so every rank must pass the window the group agreed on.
 * hist: the cell's counts per bucket, laid out [W][words][Co] (rank r's cells are one contiguous block: what a
 * reduce-scatter hands its owner); packed != 0 (n*W <= 32767 group-wide): words = NB/2, word w holds bucket w in its low
 * and bucket w + NB/2 in its high 16 bits; packed == 0: words = NB, one int32 per bucket.  Every word of the run is
 * written (cells that take no part: zero). */
int pre_dist_hist_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n, int64_t per,
                      int64_t c0, int64_t C, int64_t W, int64_t Co, const int32_t *params, int packed, int32_t *hist,
                      void *stream);

/* Every score of a taking-part cell c whose bucket is want[c][s] (want [Cp, S]: ascending, -1 = unused slot) is written to
 * send[off[c][s] + i], i < cnt[c][s] (cnt, off [Cp, S]: the caller's local counts of those buckets and their exclusive
 * scan); the order inside a list is unspecified. */
int pre_dist_collect_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n, int64_t per,
                         int64_t c0, int64_t C, int64_t W, int64_t Co, const int32_t *params, const int32_t *want, int S,
                         const int32_t *cnt, const int64_t *off, float *send, void *stream);

/* Owner side: the list of (cell co, slot s) is the W segments vals[off[w][co][s] + i], i < cnt[w][co][s] (cnt, off
 * [W, Co, S]).  For every j < nk with slot[co][j] == s (slot, rnk [Co, nk]; slot < 0: nothing to pick), out[j][co] =
 * the rnk[co][j]-th smallest (0-based, by key) score of that list.  A list longer than PRE_DIST_PICK_CAP leaves its
 * outputs untouched (the caller never sends one). */
int pre_dist_pick_f32(const float *vals, const int32_t *cnt, const int64_t *off, int64_t W, int64_t Co, int S,
                      const int32_t *slot, const int32_t *rnk, int nk, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
