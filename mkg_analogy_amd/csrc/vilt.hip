// ViLT joint embedding (reference: MarT/models/modeling_vilt.py ViltEmbeddings.forward :199-241, TextEmbeddings :260-300,
// visual_embed :112-197 with max_image_length = -1 and no pixel mask), written straight into / read straight out of the joint
// [B*S, H] residual stream, S = L + 2 (1 + P):
//   text row  t      : LN(word[id] + ttype[tt] + (t < n_tpos ? tpos[t] : 0)) + modality[0]
//   image i, token 0 : cls + ipos[0] + modality[1]
//   image i, token j : patch(b, i, perm[i][b][j-1]) + ipos[1 + perm[i][b][j-1]] + modality[1]
// The backward pass is deterministic (no float atomics): per-row LayerNorm backward and un-permuted patch gradient, then fixed-order
// column sums for every shared table, then one final fixed-order reduction of the per-position partials.
#include "common.h"
#include "mart_hip.h"

namespace {
constexpr int WPB = 4;                 // rows (waves) per workgroup
constexpr int VMAX = 4;                // float4 per lane: H <= 1024, H % 256 == 0

__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }

// one wave per row of the joint stream
__global__ __launch_bounds__(64 * WPB) void vilt_embed_fwd_k(mart_vilt_embed_desc p) {
  const int lane = threadIdx.x & 63;
  const int nv = p.H / 256, P1 = 1 + p.P, S = p.L + 2 * P1;
  const long long M = (long long)p.B * S;
  for (long long row = (long long)blockIdx.x * WPB + (threadIdx.x >> 6); row < M; row += (long long)gridDim.x * WPB) {
    const int b = (int)(row / S), t = (int)(row % S);
    float* out = p.x + row * p.H;
    if (t < p.L) {
      const long long m = (long long)b * p.L + t;
      const long long id = p.ids[m], tt = p.tt[m];
      f32x4 x[VMAX];
      float sum = 0.f;
#pragma unroll
      for (int v = 0; v < VMAX; ++v)
        if (v < nv) {
          const int c = (v * 64 + lane) * 4;
          f32x4 u = ld4(p.word + id * p.H + c);
          u += ld4(p.ttype + tt * p.H + c);
          if (t < p.n_tpos) u += ld4(p.tpos + (long long)t * p.H + c);    // modeling_vilt.py:296-299: positions stop at n_tpos
          x[v] = u;
          sum += u[0] + u[1] + u[2] + u[3];
          *(f32x4*)(p.s_text + m * p.H + c) = u;
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
      if (lane == 0) { p.mean[m] = mean; p.rstd[m] = rstd; }
#pragma unroll
      for (int v = 0; v < VMAX; ++v)
        if (v < nv) {
          const int c = (v * 64 + lane) * 4;
          const f32x4 g = ld4(p.gamma + c), be = ld4(p.beta + c), mo = ld4(p.modality + c);
          f32x4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = ((x[v][e] - mean) * rstd * g[e] + be[e]) + mo[e];
          *(f32x4*)(out + c) = y;
        }
    } else {
      const int r = t - p.L, i = r / P1, j = r % P1;
      int pi = 0;
      long long prow = -1;
      if (j > 0) {
        const int q = p.perm[((long long)i * p.B + b) * p.P + (j - 1)];
        pi = 1 + q;
        prow = ((long long)b * 2 + i) * p.P + q;
      }
      for (int v = 0; v < nv; ++v) {
        const int c = (v * 64 + lane) * 4;
        f32x4 u;
        if (j == 0) u = ld4(p.cls + c);
        else if (p.patch_f32) u = ld4(p.patch_f32 + prow * p.H + c);
        else u = bf4_to_f4(*(const bf16x4*)((const bf16*)p.patch_bf16 + prow * p.H + c));
        u += ld4(p.ipos + (long long)pi * p.H + c);
        u += ld4(p.modality + p.H + c);
        *(f32x4*)(out + c) = u;
      }
    }
  }
}

// backward, per row: text LayerNorm backward -> ds_text; image patch tokens -> dpatch (bf16, un-permuted: the weight-gradient GEMM's operand)
__global__ __launch_bounds__(64 * WPB) void vilt_embed_bwd_rows_k(mart_vilt_embed_desc p) {
  const int lane = threadIdx.x & 63;
  const int nv = p.H / 256, P1 = 1 + p.P, S = p.L + 2 * P1;
  const long long M = (long long)p.B * S;
  for (long long row = (long long)blockIdx.x * WPB + (threadIdx.x >> 6); row < M; row += (long long)gridDim.x * WPB) {
    const int b = (int)(row / S), t = (int)(row % S);
    const float* dy = p.dx + row * p.H;
    if (t < p.L) {
      const long long m = (long long)b * p.L + t;
      const float mean = p.mean[m], rstd = p.rstd[m];
      f32x4 g[VMAX], xh[VMAX];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int v = 0; v < VMAX; ++v)
        if (v < nv) {
          const int c = (v * 64 + lane) * 4;
          const f32x4 d = ld4(dy + c), ga = ld4(p.gamma + c), s = ld4(p.s_text + m * p.H + c);
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
#pragma unroll
      for (int v = 0; v < VMAX; ++v)
        if (v < nv) {
          const int c = (v * 64 + lane) * 4;
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = rstd * (g[v][e] - s1 - xh[v][e] * s2);
          *(f32x4*)(p.ds_text + m * p.H + c) = o;
        }
    } else {
      const int r = t - p.L, i = r / P1, j = r % P1;
      if (j == 0) continue;
      const int q = p.perm[((long long)i * p.B + b) * p.P + (j - 1)];
      bf16* dst = (bf16*)p.dpatch + (((long long)b * 2 + i) * p.P + q) * p.H;
      for (int v = 0; v < nv; ++v) {
        const int c = (v * 64 + lane) * 4;
        *(bf16x4*)(dst + c) = f4_to_bf4(ld4(dy + c));
      }
    }
  }
}

// backward, column sums in a fixed order.  grid (tasks, H / 256), one column per thread.  Tasks:
//   [0, P]               image position k: sum over (i, b) of the token that carries position k -> dipos[k] (k = 0: also dcls); the total
//                        also goes to ws row k (modality row 1 = sum over k, in vilt_embed_bwd_final_k)
//   [P+1, P+1+L)         text position t: sums over b of dy, dy * xhat, ds (tt = 0), ds (tt = 1) -> ws; ds also -> dtpos[t] for t < n_tpos
__global__ __launch_bounds__(256) void vilt_embed_bwd_cols_k(mart_vilt_embed_desc p) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= p.H) return;
  const int task = blockIdx.x, P1 = 1 + p.P, S = p.L + 2 * P1;
  float* ws = p.ws;
  if (task <= p.P) {
    float acc = 0.f;
    for (int i = 0; i < 2; ++i)
      for (int b = 0; b < p.B; ++b) {
        const int j = task == 0 ? 0 : 1 + p.inv[((long long)i * p.B + b) * p.P + (task - 1)];
        acc += p.dx[((long long)b * S + p.L + i * P1 + j) * p.H + c];
      }
    p.dipos[(long long)task * p.H + c] += acc;
    if (task == 0) p.dcls[c] += acc;
    ws[(long long)task * p.H + c] = acc;
  } else {
    const int t = task - P1;
    float sdy = 0.f, sxh = 0.f, st0 = 0.f, st1 = 0.f;
    for (int b = 0; b < p.B; ++b) {
      const long long m = (long long)b * p.L + t;
      const float d = p.dx[((long long)b * S + t) * p.H + c];
      const float xh = (p.s_text[m * p.H + c] - p.mean[m]) * p.rstd[m];
      const float ds = p.ds_text[m * p.H + c];
      sdy += d;
      sxh += d * xh;
      if (p.tt[m] == 0) st0 += ds; else st1 += ds;
    }
    float* w = ws + ((long long)P1 + 4LL * t) * p.H;
    w[c] = sdy; w[p.H + c] = sxh; w[2 * p.H + c] = st0; w[3 * p.H + c] = st1;
    if (t < p.n_tpos) p.dtpos[(long long)t * p.H + c] += st0 + st1;
  }
}

// final fixed-order reduction of the partials: dgamma, dbeta, dttype[0..1], dmodality[0..1]
__global__ __launch_bounds__(256) void vilt_embed_bwd_final_k(mart_vilt_embed_desc p) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.H) return;
  const int P1 = 1 + p.P;
  const float* ws = p.ws;
  float m1 = 0.f;
  for (int k = 0; k < P1; ++k) m1 += ws[(long long)k * p.H + c];
  float sdy = 0.f, sxh = 0.f, st0 = 0.f, st1 = 0.f;
  for (int t = 0; t < p.L; ++t) {
    const float* w = ws + ((long long)P1 + 4LL * t) * p.H;
    sdy += w[c]; sxh += w[p.H + c]; st0 += w[2 * p.H + c]; st1 += w[3 * p.H + c];
  }
  p.dgamma[c] += sxh;
  p.dbeta[c] += sdy;
  p.dttype[c] += st0;
  p.dttype[p.H + c] += st1;
  p.dmodality[c] += sdy;                 // text rows add modality row 0 after the LayerNorm: its gradient is dbeta's sum
  p.dmodality[p.H + c] += m1;
}

int check(const mart_vilt_embed_desc* d, bool bwd) {
  MART_CHECK(d && d->ids && d->tt && d->gamma && d->perm && d->modality, "vilt_embed: null pointer");
  MART_CHECK(d->B > 0 && d->L > 0 && d->P > 0 && d->H > 0 && d->H % 256 == 0 && d->H <= 256 * VMAX && d->n_tpos >= 0, "vilt_embed: bad shape (H % 256 == 0, H <= 1024)");
  MART_CHECK(d->s_text && d->mean && d->rstd, "vilt_embed: LayerNorm state needed");
  if (!bwd) {
    MART_CHECK(d->word && d->ttype && d->beta && d->cls && d->ipos && d->x, "vilt_embed_fwd: null pointer");
    MART_CHECK((d->patch_f32 == nullptr) != (d->patch_bf16 == nullptr), "vilt_embed_fwd: exactly one of patch_f32 / patch_bf16");
    MART_CHECK(d->n_tpos == 0 || d->tpos, "vilt_embed_fwd: text positions needed");
  } else {
    MART_CHECK(d->inv && d->dx && d->ds_text && d->dpatch && d->dgamma && d->dbeta && d->dttype && d->dcls && d->dipos && d->dmodality && d->ws,
               "vilt_embed_bwd: null pointer");
    MART_CHECK(d->n_tpos == 0 || d->dtpos, "vilt_embed_bwd: text position gradient needed");
    MART_CHECK(d->ws_bytes >= (long long)(1 + d->P + 4LL * d->L) * d->H * 4, "vilt_embed_bwd: workspace too small");
  }
  return 0;
}
}  // namespace

extern "C" int mart_vilt_embed_fwd(const mart_vilt_embed_desc* d, void* stream) {
  if (int rc = check(d, false)) return rc;
  const long long M = (long long)d->B * (d->L + 2 * (1 + d->P));
  const long long g = (M + WPB - 1) / WPB;
  hipLaunchKernelGGL(vilt_embed_fwd_k, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(64 * WPB), 0, (hipStream_t)stream, *d);
  MART_LAUNCH_CHECK();
  return 0;
}

extern "C" int mart_vilt_embed_bwd(const mart_vilt_embed_desc* d, void* stream) {
  if (int rc = check(d, true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long long M = (long long)d->B * (d->L + 2 * (1 + d->P));
  const long long g = (M + WPB - 1) / WPB;
  hipLaunchKernelGGL(vilt_embed_bwd_rows_k, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(64 * WPB), 0, st, *d);
  MART_LAUNCH_CHECK();
  hipLaunchKernelGGL(vilt_embed_bwd_cols_k, dim3(1 + d->P + d->L, (d->H + 255) / 256), dim3(256), 0, st, *d);
  MART_LAUNCH_CHECK();
  hipLaunchKernelGGL(vilt_embed_bwd_final_k, dim3((d->H + 255) / 256), dim3(256), 0, st, *d);
  MART_LAUNCH_CHECK();
  return 0;
}
