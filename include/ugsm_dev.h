/*
 * ugsm_dev.h -- entry points of libugsm_dev.so that libugsm.so does not have.
 *
 * libugsm_dev.so is the product's sources plus ug_stereomatcher_amd/csrc/dev/ (csrc/Makefile): everything include/ugsm.h declares, plus what
 * only the tests and the measurement tools need -- kernel_path 1 (one kernel per reference stage: the A/B reference of the fused kernels),
 * ugsm_config.march_min_pixels < 0 (round 1's LDS-tiled K-cost), and the probes and the range-word reader below.  A maintainer links libugsm.so.
 */
#ifndef UGSM_DEV_H
#define UGSM_DEV_H

#include "ugsm.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* The fused kernels' exact arithmetic shortcuts (f32 first quotient of PolyDisparity, x/3 by two
 * FMAs) evaluated on caller-supplied operands: delta/corr = PolyDisparity(c,l,r,thr)
 * (MatchLib.cu:805-836), third = c/3.0f for c >= 0.  Lets tests force the rare fallback branches. */
int ugsm_stage_poly_probe(ugsm_ctx *ctx, const float *d_c, const float *d_l, const float *d_r,
                          const float *d_thr, float *d_delta, float *d_corr, float *d_third, int n);

/* K-smooth's shared-reciprocal division (three weighted sums over one sumCorr, MatchLib.cu:1131-1139)
 * on caller-supplied operands, with the kernel's own range test and literal fallback:
 * q_f[i] must equal the IEEE binary32 quotient a_f[i] / s[i] bit for bit. */
int ugsm_stage_div3_probe(ugsm_ctx *ctx, const float *d_a0, const float *d_a1, const float *d_a2,
                          const float *d_s, float *d_q0, float *d_q1, float *d_q2, int n);

/* K-cost's range-guarded division (the compiler's binary32 division sequence without v_div_scale / v_div_fixup, used when
 * every pyramid value of the pair is 0 or in [2^-12, 2^9]; csrc/ugsm_exact.hpp) on caller-supplied operands:
 * q[i] must equal the IEEE binary32 quotient n[i] / d[i] bit for bit for operands that are 0 or in [2^-62, 2^37]. */
int ugsm_stage_div_probe(ugsm_ctx *ctx, const float *d_n, const float *d_d, float *d_q, int n);

/* The range words of the first n pairs of the slot's last call, read once everything enqueued on the slot has finished (the call
 * waits for the slot's stream itself): host_out[b] = 1 when some pyramid value of pair b was outside range_ok (csrc/ugsm_exact.hpp)
 * and K-cost took the compiler's division for that pair, 0 when every value passed and it took the guarded one.
 * UGSM_ERR_STATE when the slot holds no words (kernel_path 1, or no call yet), UGSM_ERR_BAD_ARG for n < 1 or n > the pairs of
 * that call. */
int ugsm_stage_range_words(ugsm_ctx *ctx, int slot, unsigned *host_out, int n);

/* 1 when the last call on the slot read level 0 of the pyramid from the images themselves (full-mode calls on rgb8 images whose level 0 is
 * matched by k_cost_march: the float level 0 is then never stored), 0 when it materialised it; minus the status (-UGSM_ERR_BAD_ARG) for a bad slot.  Host state
 * only: nothing is launched and the slot does not become busy.  The two paths give the same bits, so only this tells which one ran. */
int ugsm_stage_level0_direct(ugsm_ctx *ctx, int slot);

/* The stage-level iterate call of ugsm.h with the two images given as rgb8 (rows `stride` bytes apart) instead of float planes: the level is matched
 * the way a full-mode call matches level 0, which it reads from the images themselves -- the 8-bit instances of K-cost and of A = G * L^2 --
 * but from the caller's field d_d3, so that chosen disparities reach the clamped byte gather.  For contexts whose kernel choice gives the
 * level to k_cost_march (march_min_pixels = 1, at most 150 000 pixels); UGSM_ERR_STATE otherwise, UGSM_ERR_BAD_ARG for another input format. */
int ugsm_stage_iterate_rgb8(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int stride, float *d_d3, int W, int H,
                            int mi, int S, int is_top, int m_from, int m_to);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* UGSM_DEV_H */
