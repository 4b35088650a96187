/* mart_clip.h -- gradient clipping and gradient-norm tracking over the flat gradient buffer (libmart_hip.so, gfx950).
 *
 * An addition BESIDE the C ABI of mart_hip.h (whose version and entry-point count do not change): pl.Trainer's
 * gradient_clip_val / gradient_clip_algorithm / track_grad_norm (MarT/main.py:25, pl.Trainer.add_argparse_args), i.e.
 * torch.nn.utils.clip_grad_norm_ / clip_grad_value_ on the gradients mart_adamw is about to consume.
 *
 * Conventions are those of mart_hip.h: caller-owned buffers, everything enqueued on `stream`, no host synchronisation (the decision
 * "clip or not" never leaves the device), 0 on success, <0 on error with the text in mart_last_error() (it contains "clip").
 *
 * "The gradients" are what the AdamW chunk table names: int32 triples (start, length, flags) into `grad` (mart_adamw_desc.chunks).
 * Chunks with flag bit 2 (zero-only: a frozen tensor some launch still writes) and everything outside the table (dead tensors, padding)
 * take no part -- not read into the norm, not scaled, not clamped: torch's rule for tensors whose grad is None.  Chunk starts need no
 * alignment (16-byte accesses where the address allows, single elements at the two ends).
 *
 * Work decomposition: chunk c is cut into MART_CLIP_PARTS work items, item c * MART_CLIP_PARTS + p taking the 8192-element pieces
 * p, p + MART_CLIP_PARTS, ... of the chunk, and work item i owns partials[i].  The mapping depends on the chunk table alone and nothing is
 * combined with atomics, so every result is bit-identical from run to run and does not depend on how many workgroups were launched.
 */
#ifndef MART_CLIP_H
#define MART_CLIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MART_CLIP_PARTS 8
#define MART_CLIP_NORM_2 0   /* mode: sum of squares -> 2-norm */
#define MART_CLIP_NORM_INF 1 /* mode: max |g|        -> inf-norm */

/* number of partials mart_clip_sumsq writes for a table of n_chunks chunks (<0: n_chunks out of range) */
int mart_clip_partials_needed(int n_chunks);
/* One streaming pass over the live chunks.  mode 0: partials[i] = sum of g^2 over work item i, every square and every addition in double
 * (1e20 or 1e-30 entries neither overflow nor vanish).  mode 1: partials[i] = max |g| (a NaN survives the max).  partials[i] = 0 for a
 * skipped chunk and for needed <= i < n_partials.  Needs n_partials >= mart_clip_partials_needed(n_chunks). */
int mart_clip_sumsq(const float* grad, const int32_t* chunks, int n_chunks, int mode, double* partials, int n_partials, void* stream);
/* One workgroup combines the partials in a fixed order, in double: total = (float)(grad_scale * sqrt(sum)) (mode 0) or
 * (float)(grad_scale * max) (mode 1) -- grad_scale is the factor mart_adamw applies to the gradients later (the buffer holds the unscaled
 * sum over ranks / accumulation windows).  Then, in fp32 as torch.nn.utils.clip_grad_norm_ computes it, coef = max_norm / (total + 1e-6f)
 * -- evaluated as torch evaluates scalar / tensor, (1.0f / (total + 1e-6f)) * max_norm, so that the bits agree -- clamped to at most 1
 * (NaN stays NaN); max_norm <= 0: track only, coef = 1.  out[0] = total, out[1] = coef; log != NULL: log[log_index] = total. */
int mart_clip_finalize(const double* partials, int n_partials, int mode, float grad_scale, float max_norm, float* out /* [2] */,
                       float* log, int log_index, void* stream);
/* clip_value <= 0 (norm mode): coef = *coef_ptr is read on the device; exactly 1.0f: nothing is touched; otherwise g *= coef on the live chunks.
 * clip_value > 0 (value mode, coef_ptr may be NULL): g = clamp(g, -clip_value, clip_value), NaN stays NaN (torch.clamp).  For gradients that
 * mart_adamw scales by s > 0 later, pass clip_value / s: clamp(s g, -v, v) = s clamp(g, -v / s, v / s). */
int mart_clip_apply(float* grad, const int32_t* chunks, int n_chunks, const float* coef_ptr, float clip_value, void* stream);

#ifdef __cplusplus
}
#endif
#endif
