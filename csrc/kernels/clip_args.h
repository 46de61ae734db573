// Launch arguments of the gradient-clipping stage (csrc/kernels/clip.hip) and of the clipped
// instantiation of the tiled update (flat.hip).  Kept out of args.h / OptParams: every kernel
// includes those, and the clip parameters concern the materialised-gradient step alone.
#pragma once

namespace ea {

constexpr int CLIP_MAX_VAR = 32;    // variables: two per layer (kernel 2l, bias 2l + 1; = 2 * MAX_SEG)
constexpr int CLIP_CHUNK = 8192;    // floats of one variable per workgroup of the partial-sum kernel

struct ClipVar {
  long long off, len;   // the variable's span of a replica's row of G (len 0: absent, e.g. no bias)
  int chunk0, nch;      // its first chunk and chunk count; chunks never straddle a variable boundary
};

// Keras optimizer_v2 order: clipvalue (element clamp), then clipnorm (per variable), then
// global_clipnorm (all variables); a negative value = off
struct ClipArgs {
  const float* G; long long sG;   // [R][sG] gradient rows (sG may be odd: rows at any alignment mod 4)
  int R, nvar, nchunk;            // nchunk: chunks per replica
  float grad_scale, clipvalue, clipnorm, global_clipnorm;
  ClipVar var[CLIP_MAX_VAR];      // indexed with compile-time indices only (flat.hip find_seg)
  double* part;                   // [R][nchunk] sums of squares, one per (replica, chunk)
  float* scale;                   // [R][CLIP_MAX_VAR] out
  // a replica with no batch at this step is skipped (null ctr: every replica runs)
  const long long* ctr; const int* ntrain; int B;
};

// what the clipped update needs: g = clamp(G * grad_scale) * scale[r][2 * seg + is_bias]
struct ClipUpd {
  float clipvalue;      // < 0: no clamp
  const float* scale;   // [R][CLIP_MAX_VAR]; null: no norm clipping
};

}  // namespace ea
