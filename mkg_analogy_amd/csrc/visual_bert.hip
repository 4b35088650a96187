// VisualBERT joint embedding (reference: MarT/models/modeling_visual_bert.py VisualBertEmbeddings.forward :105-200 as MarT calls it: no
// image_text_alignment, no visual_token_type_ids), written straight into / read straight out of the joint [B*S, H] residual stream, S = L + V:
//   text row   t : word[id] + type[tt] + pos[t]
//   visual row j : proj(b, j) + vpos (visual_position_embeddings row 0) + vtype (visual_token_type_embeddings row 1)
//   x = dropout(LayerNorm(row))        one LayerNorm and one dropout over the concatenation (:198-199)
// One wave per row, H / 256 float4 per lane (the row-per-wave LayerNorm layout of norm_embed.hip).  The dropout decision of output element o = row * H + c
// is the one mart_ln_fwd / mart_text_embed_fwd take for (seed, o).  The backward pass is deterministic (no float atomics): per-row dropout + LayerNorm
// backward, then fixed-order column sums per sequence position, then one final fixed-order reduction of the per-position partials.
#include "common.h"
#include "mart_hip.h"

namespace {
constexpr int WPB = 4;                 // rows (waves) per workgroup
constexpr int VMAX = 4;                // float4 per lane: H <= 1024, H % 256 == 0

__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }

// keep factors of the four consecutive elements o .. o + 3 (o % 4 == 0): the decisions of common.h dropout_keep(seed, o + e, p), two pair hashes
__device__ __forceinline__ f32x4 keep4(uint64_t seed, uint32_t s2_lo, long long o, uint32_t thr, float inv_keep) {
  const uint64_t pair = (uint64_t)o >> 1;
  const uint32_t hi = (uint32_t)(pair >> 32);
  const uint32_t s2 = hi == 0 ? s2_lo : rng_seedmix(seed, hi);
  const uint32_t h0 = rng_pair(s2, (uint32_t)pair), h1 = rng_pair(s2, (uint32_t)pair + 1u);
  return f32x4{(h0 & 0xffffu) >= thr ? inv_keep : 0.f, (h0 >> 16) >= thr ? inv_keep : 0.f, (h1 & 0xffffu) >= thr ? inv_keep : 0.f, (h1 >> 16) >= thr ? inv_keep : 0.f};
}

__global__ __launch_bounds__(64 * WPB) void vbert_embed_fwd_k(mart_vbert_embed_desc p) {
  const int lane = threadIdx.x & 63;
  const int nv = p.H / 256, S = p.L + p.V;
  const long long M = (long long)p.B * S;
  const float inv_keep = 1.f / (1.f - p.p_drop);
  const uint32_t s2_lo = rng_seedmix(p.seed, 0), thr = dropout_thr16(p.p_drop);
  for (long long row = (long long)blockIdx.x * WPB + (threadIdx.x >> 6); row < M; row += (long long)gridDim.x * WPB) {
    const int b = (int)(row / S), t = (int)(row % S);
    const float *r0, *r1, *r2;         // the three summands, in the reference's order of addition
    if (t < p.L) {
      const long long m = (long long)b * p.L + t;
      r0 = p.word + p.ids[m] * p.H;
      r1 = p.type + p.tt[m] * p.H;
      r2 = p.pos + (long long)t * p.H;
    } else {
      r0 = p.proj + ((long long)b * p.V + (t - p.L)) * p.H;
      r1 = p.vpos;
      r2 = p.vtype;
    }
    f32x4 x[VMAX];
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < nv) {
        const int c = (v * 64 + lane) * 4;
        f32x4 u = ld4(r0 + c);
        u += ld4(r1 + c);
        u += ld4(r2 + c);
        x[v] = u;
        sum += u[0] + u[1] + u[2] + u[3];
        *(f32x4*)(p.s + row * p.H + c) = u;
      }
    const float mean = wave_sum(sum) / (float)p.H;
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < nv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = x[v][e] - mean; sq += d * d; }
      }
    const float rstd = rsqrtf(wave_sum(sq) / (float)p.H + p.eps);
    if (lane == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < nv) {
        const int c = (v * 64 + lane) * 4;
        const long long o = row * p.H + c;
        const f32x4 g = ld4(p.gamma + c), be = ld4(p.beta + c);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (x[v][e] - mean) * rstd * g[e] + be[e];
        if (p.p_drop > 0.f) y = y * keep4(p.seed, s2_lo, o, thr, inv_keep);
        *(f32x4*)(p.x + o) = y;
        if (p.x_bf16) *(bf16x4*)((bf16*)p.x_bf16 + o) = f4_to_bf4(y);
        if (p.x_f16) *(bf16x4*)((bf16*)p.x_f16 + o) = f4_to_h4raw(y);
      }
  }
}

// backward, per row: dropout backward, LayerNorm backward -> ds_text [B*L, H] (text rows), ds_vis f32 [B*V, H] + dproj bf16 [B*V, H] (visual rows)
__global__ __launch_bounds__(64 * WPB) void vbert_embed_bwd_rows_k(mart_vbert_embed_desc p) {
  const int lane = threadIdx.x & 63;
  const int nv = p.H / 256, S = p.L + p.V;
  const long long M = (long long)p.B * S;
  const float inv_keep = 1.f / (1.f - p.p_drop);
  const uint32_t s2_lo = rng_seedmix(p.seed, 0), thr = dropout_thr16(p.p_drop);
  float* ds_vis = p.ws;
  for (long long row = (long long)blockIdx.x * WPB + (threadIdx.x >> 6); row < M; row += (long long)gridDim.x * WPB) {
    const int b = (int)(row / S), t = (int)(row % S);
    const float mean = p.mean[row], rstd = p.rstd[row];
    f32x4 g[VMAX], xh[VMAX];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < nv) {
        const int c = (v * 64 + lane) * 4;
        const long long o = row * p.H + c;
        f32x4 d = ld4(p.dx + o);
        if (p.p_drop > 0.f) d = d * keep4(p.seed, s2_lo, o, thr, inv_keep);
        const f32x4 ga = ld4(p.gamma + c), s = ld4(p.s + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xh[v][e] = (s[e] - mean) * rstd;
          g[v][e] = d[e] * ga[e];
          s1 += g[v][e];
          s2 += g[v][e] * xh[v][e];
        }
      }
    s1 = wave_sum(s1) / (float)p.H;
    s2 = wave_sum(s2) / (float)p.H;
    const bool text = t < p.L;
    const long long r = text ? (long long)b * p.L + t : (long long)b * p.V + (t - p.L);
    float* dst = (text ? p.ds_text : ds_vis) + r * p.H;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
      if (v < nv) {
        const int c = (v * 64 + lane) * 4;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (g[v][e] - s1 - xh[v][e] * s2);
        *(f32x4*)(dst + c) = o;
        if (!text) *(bf16x4*)((bf16*)p.dproj + r * p.H + c) = f4_to_bf4(o);
      }
  }
}

// backward, column sums in a fixed order.  grid (S, H / 256), one column per thread; task t = sequence position: sums over b of dy, dy * xhat and of
// ds split by token type (text) / ds (visual) -> four partial rows of ws; text positions also -> dpos[t]
__global__ __launch_bounds__(256) void vbert_embed_bwd_cols_k(mart_vbert_embed_desc p) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= p.H) return;
  const int t = blockIdx.x, S = p.L + p.V;
  const float inv_keep = 1.f / (1.f - p.p_drop);
  const float* ds_vis = p.ws;
  float sdy = 0.f, sxh = 0.f, st0 = 0.f, st1 = 0.f;
  for (int b = 0; b < p.B; ++b) {
    const long long row = (long long)b * S + t, o = row * p.H + c;
    float d = p.dx[o];
    if (p.p_drop > 0.f) d = dropout_keep(p.seed, (uint64_t)o, p.p_drop) ? d * inv_keep : 0.f;
    const float xh = (p.s[o] - p.mean[row]) * p.rstd[row];
    sdy += d;
    sxh += d * xh;
    if (t < p.L) {
      const long long m = (long long)b * p.L + t;
      const float ds = p.ds_text[m * p.H + c];
      if (p.tt[m] == 0) st0 += ds; else st1 += ds;
    } else {
      st0 += ds_vis[((long long)b * p.V + (t - p.L)) * p.H + c];
    }
  }
  float* w = p.ws + ((long long)p.B * p.V + 4LL * t) * p.H;
  w[c] = sdy; w[p.H + c] = sxh; w[2 * p.H + c] = st0; w[3 * p.H + c] = st1;
  if (t < p.L) p.dpos[(long long)t * p.H + c] += st0 + st1;
}

// final fixed-order reduction of the per-position partials: dgamma, dbeta, dtype[0..1], dvpos, dvtype
__global__ __launch_bounds__(256) void vbert_embed_bwd_final_k(mart_vbert_embed_desc p) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.H) return;
  const int S = p.L + p.V;
  const float* ws = p.ws + (long long)p.B * p.V * p.H;
  float sdy = 0.f, sxh = 0.f, st0 = 0.f, st1 = 0.f, sv = 0.f;
  for (int t = 0; t < S; ++t) {
    const float* w = ws + 4LL * t * p.H;
    sdy += w[c]; sxh += w[p.H + c];
    if (t < p.L) { st0 += w[2 * p.H + c]; st1 += w[3 * p.H + c]; }
    else sv += w[2 * p.H + c];
  }
  p.dgamma[c] += sxh;
  p.dbeta[c] += sdy;
  p.dtype[c] += st0;
  p.dtype[p.H + c] += st1;
  p.dvpos[c] += sv;
  p.dvtype[c] += sv;
}

int check(const mart_vbert_embed_desc* d, bool bwd) {
  MART_CHECK(d && d->ids && d->tt && d->gamma, "vbert_embed: null pointer");
  MART_CHECK(d->B > 0 && d->L > 0 && d->V > 0 && d->H > 0 && d->H % 256 == 0 && d->H <= 256 * VMAX, "vbert_embed: bad shape (H % 256 == 0, H <= 1024)");
  MART_CHECK(d->p_drop >= 0.f && d->p_drop < 1.f, "vbert_embed: p_drop must be in [0, 1)");
  MART_CHECK(d->s && d->mean && d->rstd, "vbert_embed: LayerNorm state needed");
  if (!bwd) {
    MART_CHECK(d->word && d->pos && d->type && d->vpos && d->vtype && d->proj && d->beta && d->x, "vbert_embed_fwd: null pointer");
  } else {
    MART_CHECK(d->dx && d->ds_text && d->dproj && d->dgamma && d->dbeta && d->dpos && d->dtype && d->dvpos && d->dvtype && d->ws, "vbert_embed_bwd: null pointer");
    MART_CHECK(d->ws_bytes >= ((long long)d->B * d->V + 4LL * (d->L + d->V)) * d->H * 4, "vbert_embed_bwd: workspace too small");
  }
  return 0;
}
}  // namespace

extern "C" int mart_vbert_embed_fwd(const mart_vbert_embed_desc* d, void* stream) {
  if (int rc = check(d, false)) return rc;
  const long long M = (long long)d->B * (d->L + d->V);
  const long long g = (M + WPB - 1) / WPB;
  hipLaunchKernelGGL(vbert_embed_fwd_k, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(64 * WPB), 0, (hipStream_t)stream, *d);
  MART_LAUNCH_CHECK();
  return 0;
}

extern "C" int mart_vbert_embed_bwd(const mart_vbert_embed_desc* d, void* stream) {
  if (int rc = check(d, true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long long M = (long long)d->B * (d->L + d->V);
  const long long g = (M + WPB - 1) / WPB;
  hipLaunchKernelGGL(vbert_embed_bwd_rows_k, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(64 * WPB), 0, st, *d);
  MART_LAUNCH_CHECK();
  hipLaunchKernelGGL(vbert_embed_bwd_cols_k, dim3(d->L + d->V, (d->H + 255) / 256), dim3(256), 0, st, *d);
  MART_LAUNCH_CHECK();
  hipLaunchKernelGGL(vbert_embed_bwd_final_k, dim3((d->H + 255) / 256), dim3(256), 0, st, *d);
  MART_LAUNCH_CHECK();
  return 0;
}
