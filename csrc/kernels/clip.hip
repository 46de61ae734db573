// Gradient clipping (Keras optimizer_v2 clipnorm / global_clipnorm) on the materialised
// gradient G, between forward_backward and the tiled update (flat.hip):
//   A  clip_partial_kernel: one fp64 sum of squares per (replica, chunk of one variable)
//   B  clip_scale_kernel:   per replica, the chunks of every variable summed in a fixed order
//                           -> scale[r][t] = c / max(norm, c)
// The update then applies g = clamp(G * grad_scale) * scale[r][t].  No float atomics and no
// flags or counters to clear: every partial has one writer and every sum a fixed order, so
// the scales are bit-identical from run to run, and both launches capture into a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "clip_args.h"

namespace ea {

// NaN passes through (fminf / fmaxf would drop it): a non-finite gradient gives a
// non-finite norm and non-finite weights, as in Keras
__device__ __forceinline__ float clip_value(float v, float c) { return v < -c ? -c : (v > c ? c : v); }

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// grid (nchunk, R), 256 lanes.  Chunk c of a replica lies inside ONE variable; the table is
// walked with compile-time indices (a dynamic index into a kernarg table goes to scratch,
// flat.hip find_seg).
__global__ __launch_bounds__(256) void clip_partial_kernel(ClipArgs a) {
  __shared__ double red[4];
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (a.ctr && (long long)a.ntrain[r] - a.ctr[0] * a.B <= 0) return;   // replica has no batch this step
  long long off = a.var[0].off, len = a.var[0].len;
  int c0 = a.var[0].chunk0;
#pragma unroll
  for (int q = 1; q < CLIP_MAX_VAR; ++q) {
    if (q < a.nvar && c >= a.var[q].chunk0) {
      off = a.var[q].off;
      len = a.var[q].len;
      c0 = a.var[q].chunk0;
    }
  }
  const long long rel = (long long)(c - c0) * CLIP_CHUNK;
  const long long left = len - rel;
  const int m = left > CLIP_CHUNK ? CLIP_CHUNK : (left < 0 ? 0 : (int)left);
  const float* p = a.G + (long long)r * a.sG + off + rel;
  // scalar elements up to the first 16-byte boundary, float4 rows, scalar tail
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  if (head > m) head = m;
  const int nvec = (m - head) >> 2;
  const int tail0 = head + 4 * nvec;
  const float gs = a.grad_scale, cv = a.clipvalue;
  double acc = 0.0;
  auto add = [&](float x) {
    float v = x * gs;
    if (cv >= 0.f) v = clip_value(v, cv);
    acc += (double)(v * v);   // fp32 product, fp64 sum
  };
  if (tid < head) add(p[tid]);
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  for (int i = tid; i < nvec; i += 256) {
    const float4 x = p4[i];
    add(x.x); add(x.y); add(x.z); add(x.w);
  }
  if (tail0 + tid < m) add(p[tail0 + tid]);
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) a.part[(long long)r * a.nchunk + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (R), 256 lanes: wave w sums the partials of variables w, w + 4, ... (lane-strided,
// then the xor tree: a fixed order), then the scales
__global__ __launch_bounds__(256) void clip_scale_kernel(ClipArgs a) {
  __shared__ double tot[CLIP_MAX_VAR];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (a.ctr && (long long)a.ntrain[r] - a.ctr[0] * a.B <= 0) return;
  const double* part = a.part + (long long)r * a.nchunk;
#pragma unroll
  for (int q = 0; q < CLIP_MAX_VAR; ++q) {
    if (q < a.nvar && (q & 3) == wave) {
      const int c0 = a.var[q].chunk0, nch = a.var[q].nch;
      double s = 0.0;
      for (int i = lane; i < nch; i += 64) s += part[c0 + i];
      s = wave_sum(s);
      if (lane == 0) tot[q] = s;
    }
  }
  __syncthreads();
  if (tid >= CLIP_MAX_VAR) return;
  float* out = a.scale + (long long)r * CLIP_MAX_VAR;
  double c, ss;
  if (a.global_clipnorm >= 0.f) {   // N = sqrt(sum_t ||g_t||^2), the variables in index order
    c = (double)a.global_clipnorm;
    ss = 0.0;
    for (int t = 0; t < a.nvar; ++t) ss += tot[t];
  } else {
    c = (double)a.clipnorm;
    ss = tid < a.nvar ? tot[tid] : 0.0;
  }
  const double nrm = sqrt(ss);
  out[tid] = (float)(c / (nrm <= c ? c : nrm));   // a NaN norm stays NaN
}

}  // namespace ea

using namespace ea;

// chunk0 / nch of every variable and nchunk from the variables' (off, len); false: bad table
extern "C" int ea_clip_layout(ClipArgs* a) {
  if (a->nvar < 0 || a->nvar > CLIP_MAX_VAR) return 0;
  long long c = 0;
  for (int t = 0; t < a->nvar; ++t) {
    ClipVar& v = a->var[t];
    if (v.off < 0 || v.len < 0) return 0;
    const long long n = (v.len + CLIP_CHUNK - 1) / CLIP_CHUNK;
    if (c + n > 0x7fffffffLL) return 0;
    v.chunk0 = (int)c;
    v.nch = (int)n;
    c += n;
  }
  a->nchunk = (int)c;
  return 1;
}

// A then B on stream s (nothing when neither norm clip is set: clipvalue alone needs no norm)
extern "C" hipError_t ea_clip_scales(const ClipArgs* a, hipStream_t s) {
  const bool cn = a->clipnorm >= 0.f, gn = a->global_clipnorm >= 0.f;
  if (!cn && !gn) return hipSuccess;
  if (cn && gn) return hipErrorInvalidValue;
  if (a->R <= 0 || a->R > 65535 || !a->part || !a->scale || !a->G) return hipErrorInvalidValue;
  if (a->nchunk > 0) hipLaunchKernelGGL(clip_partial_kernel, dim3(a->nchunk, a->R), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(a->R), dim3(256), 0, s, *a);
  return hipGetLastError();
}
