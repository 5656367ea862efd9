// segment_train.hip -- training of the CT segmentation network on the device: the backward half of segment_net.hip, the Dice loss of
// the reference's driver (scripts/train_segmentation.py: SegmentationLoss(use_dice=True) on cbctmc/segmentation/losses.py: DiceLoss(
// include_background=True, reduction="none"), as cbctmc/segmentation/trainer.py: CTSegmentationTrainer reduces it) and Adam, in float32.
//
// The rule.  A batch is B samples: a rescaled patch x [P0][P1][P2] and a target t [9][P0][P1][P2] (uint8 or float32), n = P0 P1 P2.
//   Forward: exactly mcgpu_segment_run's network on one patch (NetPass::forward with segment_conv.inc's kernels).  Instance norm keeps
//     samples independent: every sample runs alone, the batch gradient is the sum of the per-sample gradients added in sample order
//     (float32).  No atomics anywhere: the same call gives the same bytes.  The reference's trainer runs its forward pass with
//     autocast disabled, so float32 without a gradient scaler is what it computes, up to the scaler's power of two.
//   Loss: p = softmax over channels 0 .. 7 of the logits z, sigmoid on channel 8 -- head_kernel's arithmetic, float64 rounded once to
//     float32.  Per sample b and channel c: I = sum t p, G = sum t, P = sum p over the voxels, float64 sums over stats_kernel's
//     segments and a 256-wide tree, the segments folded in order.  f[b][c] = 1 - (2 I + 1e-5) / (G + P + 1e-5); loss = mean of f over
//     b and c; loss_label[c] = mean of f over b.
//   Head gradient: with D = G + P + 1e-5, g[c][voxel] = (-2 t / D + (2 I + 1e-5) / D^2) / (9 B);  dL/dz_c = p_c (g_c - sum_{j<8} g_j p_j)
//     for c < 8, dL/dz_8 = g_8 p_8 (1 - p_8), in float64 and rounded once: here p, I and P are the float64 values before their
//     rounding (a second pair of sums beside the loss's; the difference g_c - sum g_j p_j would magnify the 1e-8 of the rounded
//     ones to hundreds of float32 spacings of the gradient).  1 / B is applied as speedup_train.hip
//     applies it: a sample's backward pass runs on the gradient of ITS loss (1 / 9), so that it is the same bytes in any batch, and
//     1 / B multiplies the sample's float64-folded weight gradient where it is rounded to float32 and added.
//   Backward of the net: NetPass::forward walked in reverse.
//     LeakyReLU + instance norm: speedup_train.hip's rule and kernels (unet_train_common.inc): xh recovered from y through the
//       inverse of the LeakyReLU, the two means as float64 sums, dx in float64, rounded once.
//     Convolution, weights:  dW[co][ci][tap] = sum over voxels v of dY[co][v] X~[ci][v + tap - 1], X~ what the forward stages: zero
//       outside the tensor, two channel-concatenated sources, the second through >> 1 on all three axes.
//     Convolution, bias:  db[co] = sum dY for init_conv and final_conv (float64 sums, rounded once); defined as exactly 0 for a
//       convolution that feeds an instance norm (mathematically 0; autograd gives rounding noise there) -- those biases never move.
//     Convolution, input:  the padding is zeros, so the adjoint is the forward convolution itself run on dY with the weights transposed
//       in (co, ci) and flipped in the taps; there is no border to fold.  Channels of the first source are the skip's gradient;
//       channels of the second are summed over each 2 x 2 x 2 block into the half-size gradient (the adjoint of the nearest upsample;
//       float64, rounded once).  init_conv needs none.
//     Max-pool:  the gradient goes to the first maximal element of the 2 x 2 x 2 window in scan order (d0 outermost, d2 innermost:
//       torch's rule), recomputed from the saved input, and is added to what the decoder path left in the skip's gradient.
//   Adam (no weight decay): unet_train_common.inc's kernel, speedup_train.hip's rule; the learning rate is an argument of every step
//     (the host's plateau scheduler owns it), nothing decays on the device.
//
// The kernels.
//   conv3d_wgrad_mfma_kernel: a GEMM on v_mfma_f32_32x32x2_f32 with M = C_out, N = C_in per tap, K = voxels.  27 accumulators of 16
//     registers do not fit, so a workgroup of 4 waves owns ONE dz (9 taps, 9 accumulators, as the 2-D kernel), 32 output x 32 input
//     channels and a range of voxel tiles; dz is part of the grid.  With dz fixed, a 1 x 4 x 32 tile of dY in plane z needs only plane
//     z + dz - 1 of X: the 2-D kernel's LDS layout carries over (6 x 34 halo of 32 input channels beside the 4 x 32 tile of 32 dY
//     channels, odd channel strides 205 and 129, so that the 32 channels a wave reads at one voxel lie in 32 banks); what changes is
//     masking to zero instead of clamping, and the loop over planes -- a tile whose X plane lies outside the tensor is skipped
//     (uniform over the workgroup).  One MFMA k-step is two neighbouring voxels along d2; the nine taps are nine accumulators fed from
//     one dY value and nine shifted reads.  K is split across workgroups and waves into float32 partials [partial][C_out][C_in][27]
//     (the three dz workgroups of a split write disjoint taps of the same partial); wgrad_fold_kernel adds them in float64 in the
//     order of the partials and rounds once.
//     Resources (compiler's report, gfx950; `make resources`): 35 VGPRs + 144 AGPRs (the nine accumulators), 74 SGPRs, no scratch,
//     LDS 42,752 B per workgroup (X 32 x 205 floats = 26,240 B, dY 32 x 129 floats = 16,512 B): the registers hold 2 waves per SIMD,
//     so 2 workgroups are resident per CU.
//   Input gradient: conv3x3x3_mfma_kernel of segment_conv.inc with a second packing (pack_dgrad_weights_kernel: transposed, taps
//     flipped), one packing per source of the layer: the first source's channels are written straight into the skip's gradient, the
//     second's into one [c2][D] buffer that upsample_backward_kernel sums into the half-size gradient.  A full-size gradient of the
//     concatenated 64 channels never exists, and no copy kernel hands the first channels over.
//   maxpool3d_backward_kernel, dice_sums_kernel + dice_fold_kernel, head_grad_kernel, target_kernel (uint8 -> float32).
// The weights, both moments, both packings and all buffers of a pass live on the device between steps behind a handle; both packings
// are redone on the device after each update.
#include <chrono>
#include <memory>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

constexpr int kTaps = 27;
#include "unet_common.inc"
#include "segment_conv.inc"
#include "unet_train_common.inc"

constexpr int kMaxLevels = 8;
constexpr int kClasses = 9;

// ------------------------------------------------------------------------------------------------ convolution, weight gradient
constexpr int kWgH = 4, kWgW = 32;                           // d1 rows (one per wave) and d2 columns of a voxel tile
constexpr int kWgHaloW = kWgW + 2;
constexpr int kWgHalo = (kWgH + 2) * kWgHaloW;               // 204
constexpr int kWgXStride = kWgHalo + 1, kWgYStride = kWgH * kWgW + 1;  // odd: 32 channels at one voxel lie in 32 banks
constexpr int kWgTarget = 500;                               // workgroups to aim for when K is split

struct WgradArgs {
  const float* src1;  // [c1][D0][D1][D2]
  const float* src2;  // [c2][E0][E1][E2] or nullptr
  int c1, c2, D0, D1, D2, E0, E1, E2, ups;
  const float* dy;    // [c_out][D0][D1][D2]
  int c_out;
  float* part;        // [4 splits][c_out][c1 + c2][27]
  int tiles_x, tiles_y, n_tiles, tiles_per_split, splits;
};

__global__ __launch_bounds__(256) void conv3d_wgrad_mfma_kernel(WgradArgs a) {
  __shared__ float s_x[32 * kWgXStride];
  __shared__ float s_dy[32 * kWgYStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int split = (int)(blockIdx.x % (unsigned)a.splits), dz = (int)(blockIdx.x / (unsigned)a.splits), cob = blockIdx.y, cib = blockIdx.z;
  const int c_in = a.c1 + a.c2;
  const size_t n1 = ((size_t)a.D0 * a.D1) * a.D2, n2 = ((size_t)a.E0 * a.E1) * a.E2;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* pa = s_dy + col * kWgYStride + wave * kWgW + h;      // A[co = col][voxel 2 k + h] of the wave's row
  const float* pb = s_x + col * kWgXStride + wave * kWgHaloW + h;   // B[voxel][ci = col]
  const int t_end = min((split + 1) * a.tiles_per_split, a.n_tiles);
  for (int t = split * a.tiles_per_split; t < t_end; ++t) {
    const int tx = t % a.tiles_x, tr = t / a.tiles_x, ty = tr % a.tiles_y, z = tr / a.tiles_y;
    const int zs = z + dz - 1;                 // the plane of X that plane z of dY meets under this dz
    if (zs < 0 || zs >= a.D0) continue;        // zero padding: nothing to add (uniform over the workgroup)
    const int x0 = tx * kWgW, y0 = ty * kWgH;
    __syncthreads();  // the reads of the tile before
    for (int e = tid; e < 32 * kWgHalo; e += 256) {
      const int c = e / kWgHalo, r = e - c * kWgHalo, yy = r / kWgHaloW, xx = r - yy * kWgHaloW;
      const int gc = cib * 32 + c;
      const int y = y0 + yy - 1, x = x0 + xx - 1;
      float v = 0.f;
      if (y >= 0 && y < a.D1 && x >= 0 && x < a.D2) {
        if (gc < a.c1) v = a.src1[(size_t)gc * n1 + ((size_t)zs * a.D1 + y) * a.D2 + x];
        else if (gc < c_in) v = a.src2[(size_t)(gc - a.c1) * n2 + ((size_t)(zs >> a.ups) * a.E1 + (y >> a.ups)) * a.E2 + (x >> a.ups)];
      }
      s_x[c * kWgXStride + r] = v;
    }
    for (int e = tid; e < 32 * kWgH * kWgW; e += 256) {
      const int c = e / (kWgH * kWgW), r = e - c * (kWgH * kWgW), yy = r / kWgW, xx = r - yy * kWgW;
      const int co = cob * 32 + c, y = y0 + yy, x = x0 + xx;
      s_dy[c * kWgYStride + r] = (co < a.c_out && y < a.D1 && x < a.D2) ? a.dy[(size_t)co * n1 + ((size_t)z * a.D1 + y) * a.D2 + x] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kWgW / 2; ++k) {
      const float av = pa[2 * k];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float bv = pb[(tap / 3) * kWgHaloW + 2 * k + tap % 3];
        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tap], 0, 0, 0);
      }
    }
  }
  const int ci = cib * 32 + col;
  if (ci >= c_in) return;
  float* out = a.part + (size_t)(split * 4 + wave) * ((size_t)a.c_out * c_in * 27);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = cob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;  // the 32x32 C/D map: row of register r in lane half h
    if (co < a.c_out) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) out[((size_t)co * c_in + ci) * 27 + dz * 9 + tap] = acc[tap][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------- convolution, input gradient
// The forward packing (unet_common.inc: pack_weights_kernel) of W'[co][ci0 + j][tap] -> [input channel co][output channel j][26 - tap]:
// the GEMM's input channels are the layer's output channels, its output channels the cn input channels of the layer from ci0 on
__global__ __launch_bounds__(256) void pack_dgrad_weights_kernel(const float* w, float* wpack, int c_in, int c_out, int ci0, int cn, int n_chunks,
                                                                 size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int out_local = (int)(e % 32);
  size_t r = e / 32;
  const int kk = (int)(r % kKK);
  r /= kKK;
  const int ch = (int)(r % n_chunks), cb = (int)(r / n_chunks);
  const int hh = kk & 1, tap = (kk >> 1) % kTaps, cp = (kk >> 1) / kTaps;
  const int co = ch * kCK + cp * 2 + hh, j = cb * 32 + out_local;  // of the layer
  wpack[e] = (j < cn && co < c_out) ? w[((size_t)co * c_in + ci0 + j) * kTaps + (kTaps - 1 - tap)] : 0.f;
}

// out [C][E] = the sum of each 2 x 2 x 2 block of ext [C][D] (E = (D + 1) / 2), in float64 in scan order, rounded once
__global__ __launch_bounds__(256) void upsample_backward_kernel(const float* ext, int C, int D0, int D1, int D2, int E0, int E1, int E2, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ((size_t)C * E0 * E1) * E2) return;
  const int x2 = (int)(i % E2), y2 = (int)((i / E2) % E1);
  const size_t cz = i / ((size_t)E2 * E1);
  const int z2 = (int)(cz % E0), c = (int)(cz / E0);
  const float* p = ext + ((size_t)c * D0) * D1 * D2;
  double s = 0.0;
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int z = 2 * z2 + dz, y = 2 * y2 + dy, x = 2 * x2 + dx;
        if (z < D0 && y < D1 && x < D2) s += (double)p[((size_t)z * D1 + y) * D2 + x];
      }
  out[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------ small kernels
// dx[first maximum of the 2 x 2 x 2 window in scan order] += dy
__global__ __launch_bounds__(256) void maxpool3d_backward_kernel(const float* x, const float* dy, float* dx, int C, int D0, int D1, int D2) {
  const int O0 = D0 >> 1, O1 = D1 >> 1, O2 = D2 >> 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ((size_t)C * O0 * O1) * O2) return;
  const int xo = (int)(i % O2), yo = (int)((i / O2) % O1);
  const size_t cz = i / ((size_t)O2 * O1);
  const int zo = (int)(cz % O0), c = (int)(cz / O0);
  const size_t base = (((size_t)c * D0 + 2 * zo) * D1 + 2 * yo) * D2 + 2 * xo;
  const size_t sy = (size_t)D2, sz = (size_t)D1 * D2;
  const size_t off[8] = {0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1};
  const float* p = x + base;
  float m = p[0];
  size_t at = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const float v = p[off[k]];
    if (v > m) {
      m = v;
      at = off[k];
    }
  }
  dx[base + at] += dy[i];
}

__global__ __launch_bounds__(256) void target_kernel(const unsigned char* raw, float* t, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = (float)raw[i];
}

// part[s][c][0 .. 4] = (I, P of p rounded once to float32; G; I, P of p as float64) of segment s of channel c of one sample: float64
// sums, the 256-wide tree.  The loss is stated on the rounded p (what head_kernel gives); its gradient is taken where p is not yet
// rounded: the two differ by 1e-8 relative, which the difference g_c - sum g_j p_j would magnify to hundreds of float32 spacings.
// The 45 sums of a thread go through one 256-double tree each, one after the other: at most 64 workgroups run this once per sample
// (3 of the step's 133 ms at 384 x 384 x 64 lie in the whole loss), so the plain form of stats_kernel's tree was kept; a wave-level
// reduction first would cut the barriers, not the float64 exponentials that dominate.  head_grad_kernel evaluates head_of again
// instead of reading nine float64 probabilities per voxel back from memory.
constexpr int kDiceSums = 5;
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* logits, const float* t, size_t n, int S, double* part) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const Segment g = segment_of(n, S, s);
  double acc[kDiceSums * kClasses];
#pragma unroll
  for (int k = 0; k < kDiceSums * kClasses; ++k) acc[k] = 0.0;
  for (size_t i = g.lo + tid; i < g.hi; i += 256) {
    double p[kClasses];
    head_of(logits, n, i, p);
#pragma unroll
    for (int c = 0; c < kClasses; ++c) {
      const double tv = (double)t[(size_t)c * n + i], pc = (double)(float)p[c];
      acc[kDiceSums * c] += tv * pc;
      acc[kDiceSums * c + 1] += pc;
      acc[kDiceSums * c + 2] += tv;
      acc[kDiceSums * c + 3] += tv * p[c];
      acc[kDiceSums * c + 4] += p[c];
    }
  }
#pragma unroll
  for (int k = 0; k < kDiceSums * kClasses; ++k) {
    const double total = block_tree(acc[k]);
    if (tid == 0) part[(size_t)s * (kDiceSums * kClasses) + k] = total;
  }
}

// f[c] (from the rounded p) and coef[c] = (D, 2 I + 1e-5) (from p as float64) of one sample: the segments folded in order
__global__ void dice_fold_kernel(const double* part, int S, double* f, double2* coef) {
  const int c = threadIdx.x;
  if (c >= kClasses) return;
  double v[kDiceSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < S; ++s) {
    const double* q = part + (size_t)s * (kDiceSums * kClasses) + kDiceSums * c;
#pragma unroll
    for (int k = 0; k < kDiceSums; ++k) v[k] += q[k];
  }
  f[c] = 1.0 - (2.0 * v[0] + 1e-5) / (v[2] + v[1] + 1e-5);
  coef[c] = make_double2(v[2] + v[4] + 1e-5, 2.0 * v[3] + 1e-5);
}

// g [9][n] = dL/d logits of one sample; scale = 1 / (9 B) (the trainer: 1 / 9, its 1 / B is applied where the weight gradient is added)
__global__ __launch_bounds__(256) void head_grad_kernel(const float* logits, const float* t, const double2* coef, size_t n, double scale, float* g) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double p[kClasses], gc[kClasses], dot = 0.0;
  head_of(logits, n, i, p);
#pragma unroll
  for (int c = 0; c < kClasses; ++c) {
    const double D = coef[c].x, num = coef[c].y;
    gc[c] = (-2.0 * (double)t[(size_t)c * n + i] / D + num / (D * D)) * scale;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) dot += gc[c] * p[c];
#pragma unroll
  for (int c = 0; c < 8; ++c) g[(size_t)c * n + i] = (float)(p[c] * (gc[c] - dot));
  g[8 * n + i] = (float)(gc[8] * p[8] * (1.0 - p[8]));
}

// -------------------------------------------------------------------------------------------------------------------- host
using Report = mcgpu_segment_train_report;

std::string triple(const int* v) { return std::to_string(v[0]) + " x " + std::to_string(v[1]) + " x " + std::to_string(v[2]); }

// how K of a layer's weight gradient is split: tiles of 1 x 4 x 32 voxels per workgroup, 4 partials (waves) per workgroup
struct WgradPlan {
  int tiles_x, tiles_y, n_tiles, tiles_per_split, splits;
  int partials() const { return 4 * splits; }
};
WgradPlan wgrad_plan(int c_in, int c_out, const Dims& D) {
  WgradPlan p;
  p.tiles_x = (D.d[2] + kWgW - 1) / kWgW;
  p.tiles_y = (D.d[1] + kWgH - 1) / kWgH;
  p.n_tiles = p.tiles_x * p.tiles_y * D.d[0];
  const int blocks = 3 * ((c_out + 31) / 32) * ((c_in + 31) / 32);
  const int want = std::min(p.n_tiles, std::max(1, (kWgTarget + blocks - 1) / blocks));
  p.tiles_per_split = (p.n_tiles + want - 1) / want;
  p.splits = (p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}
size_t wgrad_part_floats(int c_in, int c_out, const Dims& D) { return (size_t)wgrad_plan(c_in, c_out, D).partials() * c_out * c_in * kTaps; }

// grad_w [c_out][c_in][27] += scale dW; grad_b [c_out] += scale db when grad_b
void launch_wgrad(RunnerBase<Report>& R, int c_out, const float* src1, int c1, const float* src2, int c2, int ups, const Dims& D, const float* dy, float* part,
                  float* grad_w, float* grad_b, double scale) {
  const Dims E = ups ? D.halved_up() : D;
  const WgradPlan p = wgrad_plan(c1 + c2, c_out, D);
  WgradArgs a;
  a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = c2; a.ups = ups ? 1 : 0;
  a.D0 = D.d[0]; a.D1 = D.d[1]; a.D2 = D.d[2]; a.E0 = E.d[0]; a.E1 = E.d[1]; a.E2 = E.d[2];
  a.dy = dy; a.c_out = c_out; a.part = part;
  a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.n_tiles = p.n_tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;
  hipLaunchKernelGGL(conv3d_wgrad_mfma_kernel, dim3((unsigned)(3 * p.splits), (unsigned)((c_out + 31) / 32), (unsigned)((c1 + c2 + 31) / 32)), dim3(256), 0,
                     nullptr, a);
  launch_wgrad_fold(part, p.partials(), (size_t)c_out * (c1 + c2) * kTaps, grad_w, dy, c_out, D.voxels(), R.d_part, grad_b, scale);
}

// The input-gradient GEMMs of a layer, one per source: their input channels are the layer's output channels
struct Dgrad {
  ConvLayer first, second;  // second.c_out = 0: the layer has one source; first.c_out = 0: none
  int ci0 = 0;              // where the second source's channels begin
  Dgrad() = default;
  Dgrad(const ConvLayer& l, int c1) : first(gemm(l, c1)), second(gemm(l, l.c_in - c1)), ci0(c1) {}
  static ConvLayer gemm(const ConvLayer& l, int cn) {
    ConvLayer d;
    d.c_in = l.c_out;
    d.c_out = cn;
    d.nb = 1;
    d.n_chunks = (d.c_in + kCK - 1) / kCK;
    return d;
  }
  template <class F>
  void each(F f) {
    if (first.c_out) f(first);
    if (second.c_out) f(second);
  }
  void pack(const ConvLayer& l, const float* d_w) const {
    pack_one(l, first, 0, d_w);
    pack_one(l, second, ci0, d_w);
  }
  static void pack_one(const ConvLayer& l, const ConvLayer& d, int ci0, const float* d_w) {
    const size_t total = d.pack_floats();
    if (total) hipLaunchKernelGGL(pack_dgrad_weights_kernel, dim3(blocks_of(total)), dim3(256), 0, nullptr, d_w, d.wpack, l.c_in, l.c_out, ci0, d.c_out, d.n_chunks, total);
  }
};
// of the second source at full size, before it is summed into the half-size gradient
size_t dgrad_ext_floats(const ConvLayer& l, int c1, const Dims& D) { return (size_t)(l.c_in - c1) * D.voxels(); }

// out1 [c1][D] and out2 [c2][D or its half] = the gradient of the layer's two sources; ext: room for [c2][D] when ups
void launch_dgrad(const Dgrad& d, const float* dy, const Dims& D, float* ext, int ups, float* out1, float* out2) {
  launch_conv(d.first, dy, d.first.c_in, nullptr, 0, D, out1);
  if (!d.second.c_out) return;
  if (!ups) {
    launch_conv(d.second, dy, d.second.c_in, nullptr, 0, D, out2);
    return;
  }
  const Dims E = D.halved_up();
  launch_conv(d.second, dy, d.second.c_in, nullptr, 0, D, ext);
  const size_t n = (size_t)d.second.c_out * E.voxels();
  hipLaunchKernelGGL(upsample_backward_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, ext, d.second.c_out, D.d[0], D.d[1], D.d[2], E.d[0], E.d[1], E.d[2], out2);
}

void launch_maxpool_backward(const float* x, const float* dy, float* dx, int C, const Dims& D) {
  const size_t n = (size_t)C * D.shifted(1).voxels();
  if (n) hipLaunchKernelGGL(maxpool3d_backward_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, dy, dx, C, D.d[0], D.d[1], D.d[2]);
}

// f [9] and coef [9] of one sample's logits against its target
void launch_dice(const float* logits, const float* t, size_t n, double* d_dice, double* d_f, double2* d_coef) {
  const int S = segments_of(n);
  hipLaunchKernelGGL(dice_sums_kernel, dim3((unsigned)S), dim3(256), 0, nullptr, logits, t, n, S, d_dice);
  hipLaunchKernelGGL(dice_fold_kernel, dim3(1), dim3(64), 0, nullptr, d_dice, S, d_f, d_coef);
}

#include "unet_train_host.inc"

}  // namespace

struct mcgpu_segment_trainer {
  mcgpu_segment_train_options o;
  TrainRunner R;
  Dims P;
  TrainCore core;
  size_t n = 0;  // voxels of a patch
  float *d_x = nullptr, *d_t = nullptr;
  unsigned char* d_traw = nullptr;
  double2* d_coef = nullptr;
  double *d_dice = nullptr, *d_f = nullptr;
  std::unique_ptr<TrainNet> net;
  unsigned long long step = 0;
};

namespace {

using Trainer = mcgpu_segment_trainer;

void check_create(const char* fn, const mcgpu_segment_train_options& o) {
  if (!o.weights) refuse(fn, "weights is NULL");
  if (o.max_batch < 1) refuse(fn, "max_batch is " + std::to_string(o.max_batch) + ", expected >= 1");
  for (int a = 0; a < 3; ++a)
    if (o.patch_shape[a] < 1) refuse(fn, "patch_shape must be >= 1: " + triple(o.patch_shape));
  if (o.levels < 1 || o.levels > kMaxLevels) refuse(fn, "levels is " + std::to_string(o.levels) + ", expected 1.." + std::to_string(kMaxLevels));
  const int L = o.levels;
  for (int i = 0; i < 2 * L + 2; ++i)
    if (o.n_filters[i] < 1 || o.n_filters[i] > 65535) refuse(fn, "n_filters[" + std::to_string(i) + "] is " + std::to_string(o.n_filters[i]) + ", expected 1..65535");
  if (o.n_classes != kClasses)
    refuse(fn, "the final convolution has " + std::to_string(o.n_classes) + " outputs, expected 9 (8 softmax labels and the lung vessels)");
  if (o.n_filters[2 * L + 1] != o.n_filters[2 * L])
    refuse(fn, "inconsistent weight shapes: final_conv takes " + std::to_string(o.n_filters[2 * L + 1]) + " channels but dec_0 gives " + std::to_string(o.n_filters[2 * L]));
  size_t expect = 0;
  NetLayers(1, L, o.n_filters, o.n_classes, expect);
  if (o.n_weights != expect)
    refuse(fn, "inconsistent weight shapes: n_weights is " + std::to_string(o.n_weights) + " but the architecture has " + std::to_string(expect) + " values");
  for (int a = 0; a < 3; ++a)
    if (o.patch_shape[a] % (1 << L))
      refuse(fn, "patch axis " + std::to_string(a) + " is " + std::to_string(o.patch_shape[a]) + ", not divisible by " + std::to_string(1 << L) + " (2^levels)");
  if (o.patch_shape[0] > 2 * 65535 || o.patch_shape[1] > 4 * 65535 || ((size_t)o.patch_shape[0] * o.patch_shape[1]) * o.patch_shape[2] > 0x7fffffffull)
    refuse(fn, "a patch of " + triple(o.patch_shape) + " is too large: at most 2^31 - 1 voxels");
  if (((size_t)(o.patch_shape[0] >> L) * (o.patch_shape[1] >> L)) * (o.patch_shape[2] >> L) < 2)
    refuse(fn, "the bottleneck of a " + triple(o.patch_shape) + " patch has fewer than 2 voxels: instance norm is undefined");
  if (!(o.beta1 >= 0.0 && o.beta1 < 1.0) || !(o.beta2 >= 0.0 && o.beta2 < 1.0))
    refuse(fn, "beta1 and beta2 must be in [0, 1): " + std::to_string(o.beta1) + ", " + std::to_string(o.beta2));
}

void check_batch(const char* fn, const Trainer* T, int n, const float* image, const void* target, int target_type, bool need_target) {
  if (!T) refuse(fn, "handle is NULL");
  if (n < 1 || n > T->o.max_batch) refuse(fn, "n is " + std::to_string(n) + " but the trainer was created for 1.." + std::to_string(T->o.max_batch));
  if (!image) refuse(fn, "image is NULL");
  if (need_target) {
    if (!target) refuse(fn, "target is NULL");
    if (target_type != MCGPU_TARGET_UINT8 && target_type != MCGPU_TARGET_FLOAT32)
      refuse(fn, "target_type " + std::to_string(target_type) + ": MCGPU_TARGET_UINT8 or MCGPU_TARGET_FLOAT32");
  }
}

// logits of sample p on the device (net->act->out), every layer's output and sums kept for the backward
const float* forward_sample(Trainer& T, const float* image, int p) {
  HIP_TRY(hipMemcpy(T.d_x, image + (size_t)p * T.n, T.n * 4, hipMemcpyHostToDevice));
  T.R.norm_parts = &T.net->parts;
  T.R.norm_i = 0;
  const float* logits = T.net->act->forward(T.d_x);
  T.R.norm_parts = nullptr;
  return logits;
}

void upload_target(Trainer& T, const void* target, int target_type, int p) {
  const size_t m = (size_t)kClasses * T.n;
  if (target_type == MCGPU_TARGET_FLOAT32) {
    HIP_TRY(hipMemcpy(T.d_t, (const float*)target + (size_t)p * m, m * 4, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(T.d_traw, (const unsigned char*)target + (size_t)p * m, m, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(target_kernel, dim3(blocks_of(m)), dim3(256), 0, nullptr, T.d_traw, T.d_t, m);
  }
}

// forward of every sample, its f, and (with `gradient`) its gradient of the loss added to d_grad; f [n][9] comes back to the host
void run_batch(Trainer& T, int n, const float* image, const void* target, int target_type, bool gradient, std::vector<double>& f) {
  TrainRunner& R = T.R;
  // A sample's backward pass runs on the gradient of ITS loss (1 / 9) and is the same bytes in any batch; the share 1 / B of the
  // batch is applied where the sample's gradient is rounded to float32 and added to the batch's
  const double inv_b = 1.0 / (double)n;
  if (gradient) HIP_TRY(hipMemset(T.core.d_grad, 0, T.core.n_w * 4));
  for (int p = 0; p < n; ++p) {
    const float* logits = nullptr;
    {
      Stage st(R.dev, R.rep.ms_forward);
      logits = forward_sample(T, image, p);
      upload_target(T, target, target_type, p);
      launch_dice(logits, T.d_t, T.n, T.d_dice, T.d_f + (size_t)p * kClasses, T.d_coef);
      st.done();
    }
    if (!gradient) continue;
    {
      Stage st(R.dev, R.rep.ms_dgrad);
      hipLaunchKernelGGL(head_grad_kernel, dim3(blocks_of(T.n)), dim3(256), 0, nullptr, logits, T.d_t, T.d_coef, T.n, 1.0 / (double)kClasses, T.net->grad->out);
      st.done();
    }
    backward_sample(R, *T.net, T.d_x, T.core, inv_b);
  }
  f.resize((size_t)n * kClasses);
  HIP_TRY(hipMemcpy(f.data(), T.d_f, f.size() * sizeof(double), hipMemcpyDeviceToHost));  // once per batch; waits for the device
}

// loss = mean of f over samples and labels, loss_label[c] = mean over samples: samples in order, labels in order
void fill_losses(Report& r, int n, const double* f) {
  double all = 0.0;
  for (int c = 0; c < kClasses; ++c) r.loss_label[c] = 0.0;
  for (int b = 0; b < n; ++b)
    for (int c = 0; c < kClasses; ++c) {
      all += f[(size_t)b * kClasses + c];
      r.loss_label[c] += f[(size_t)b * kClasses + c];
    }
  for (int c = 0; c < kClasses; ++c) r.loss_label[c] /= (double)n;
  r.loss = all / ((double)n * kClasses);
  r.n = n;
}

void fill_report(Trainer& T, int n, const std::vector<double>& f, const std::chrono::steady_clock::time_point& t0, Report* report) {
  Report& r = T.R.rep;
  fill_losses(r, n, f.data());
  r.step = T.step;
  finish_report(T.R, t0, report);
}

}  // namespace

extern "C" int mcgpu_segment_train_create(const mcgpu_segment_train_options* caller_o, mcgpu_segment_trainer** handle) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_create";
  if (!handle) refuse(fn, "handle is NULL");
  *handle = nullptr;
  std::unique_ptr<Trainer> T(new Trainer);
  mcgpu::read_options(fn, "mcgpu_segment_train_options", caller_o, T->o);
  const mcgpu_segment_train_options& o = T->o;
  check_create(fn, o);
  TrainRunner& R = T->R;
  R.dry = o.dry != 0;
  T->P = Dims{{o.patch_shape[0], o.patch_shape[1], o.patch_shape[2]}};
  T->n = T->P.voxels();
  size_t cursor = 0;
  NetLayers layers(1, o.levels, o.n_filters, o.n_classes, cursor);
  const int widest = std::max(kClasses, layers.widest());
  R.init(o.device, widest);
  TrainCore& C = T->core;
  C.alloc(R, o.device, o.weights, (size_t)o.n_weights, widest);
  T->d_x = R.alloc(T->n);
  T->d_t = R.alloc((size_t)kClasses * T->n);
  T->d_traw = (unsigned char*)R.alloc_bytes((size_t)kClasses * T->n, true);
  T->d_dice = (double*)R.alloc_bytes((size_t)kMaxSegments * kDiceSums * kClasses * sizeof(double), true);
  T->d_f = (double*)R.alloc_bytes((size_t)o.max_batch * kClasses * sizeof(double), true);
  T->d_coef = (double2*)R.alloc_bytes((size_t)kClasses * sizeof(double2), true);
  T->net.reset(new TrainNet(std::move(layers), R, T->P, C.d_w, C.d_zero));
  C.alloc_scratch(T->net->part_floats, T->net->ext_floats);
  if (!R.dry) C.repack({T->net.get()});
  *handle = T.release();
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_step(mcgpu_segment_trainer* T, int n, const float* image, const void* target, int target_type, double lr, int update,
                                        mcgpu_segment_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_step";
  check_batch(fn, T, n, image, target, target_type, true);
  if (update && !(lr > 0.0)) refuse(fn, "lr is " + std::to_string(lr) + ", expected > 0");
  mcgpu::check_report(fn, "report", "mcgpu_segment_train_report", report);
  T->core.check_live(fn);
  const auto t0 = std::chrono::steady_clock::now();
  clear_times(T->R.rep);
  std::vector<double> f;
  run_batch(*T, n, image, target, target_type, update != 0, f);
  if (update) {
    Stage st(T->R.dev, T->R.rep.ms_optimizer);
    ++T->step;
    T->core.update(*T->net, lr, T->o.beta1, T->o.beta2, T->step);
    st.done();
  }
  fill_report(*T, n, f, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_gradients(mcgpu_segment_trainer* T, int n, const float* image, const void* target, int target_type, float* flat_gradient,
                                             mcgpu_segment_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_gradients";
  check_batch(fn, T, n, image, target, target_type, true);
  if (!flat_gradient) refuse(fn, "flat_gradient is NULL");
  mcgpu::check_report(fn, "report", "mcgpu_segment_train_report", report);
  T->core.check_live(fn);
  const auto t0 = std::chrono::steady_clock::now();
  clear_times(T->R.rep);
  std::vector<double> f;
  run_batch(*T, n, image, target, target_type, true, f);
  HIP_TRY(hipMemcpy(flat_gradient, T->core.d_grad, T->core.n_w * 4, hipMemcpyDeviceToHost));
  fill_report(*T, n, f, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_predict(mcgpu_segment_trainer* T, int n, const float* image, float* logits) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_predict";
  check_batch(fn, T, n, image, nullptr, 0, false);
  if (!logits) refuse(fn, "logits is NULL");
  T->core.check_live(fn);
  const size_t m = (size_t)kClasses * T->n;
  for (int p = 0; p < n; ++p) {
    const float* d_logits = forward_sample(*T, image, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(logits + (size_t)p * m, d_logits, m * 4, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_get_state(mcgpu_segment_trainer* T, mcgpu_segment_train_state* caller_s) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_get_state";
  if (!T) refuse(fn, "handle is NULL");
  mcgpu_segment_train_state s;
  mcgpu::read_options(fn, "mcgpu_segment_train_state", caller_s, s);
  T->core.check_state(fn, s);
  T->core.get_arrays(fn, s);
  s.n_weights = T->core.n_w;
  s.step = T->step;
  s.planned_device_bytes = T->core.planned_bytes();
  mcgpu::write_report(caller_s, s);
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_set_state(mcgpu_segment_trainer* T, const mcgpu_segment_train_state* caller_s) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_set_state";
  if (!T) refuse(fn, "handle is NULL");
  mcgpu_segment_train_state s;
  mcgpu::read_options(fn, "mcgpu_segment_train_state", caller_s, s);
  T->core.check_state(fn, s);
  T->core.set_arrays(fn, s, {T->net.get()});
  T->step = s.step;
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_destroy(mcgpu_segment_trainer* T) {
  ABI_BEGIN
  if (!T) return 0;
  if (!T->R.dry) (void)hipSetDevice(T->o.device);
  delete T;
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_train_stage(int stage, const mcgpu_segment_train_stage_args* caller_a, mcgpu_segment_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_train_stage";
  mcgpu_segment_train_stage_args a;
  mcgpu::read_options(fn, "mcgpu_segment_train_stage_args", caller_a, a);
  mcgpu::check_report(fn, "report", "mcgpu_segment_train_report", report);
  if (stage < MCGPU_SEGMENT_TRAIN_STAGE_CONV_WGRAD || stage > MCGPU_SEGMENT_TRAIN_STAGE_LOSS) refuse(fn, "unknown stage " + std::to_string(stage));
  if (!a.in || !a.out) refuse(fn, "in or out is NULL");
  for (int i = 0; i < 3; ++i)
    if (a.shape[i] < 1) refuse(fn, "shape must be >= 1: " + triple(a.shape));
  const Dims D{{a.shape[0], a.shape[1], a.shape[2]}};
  const size_t n = D.voxels();
  if ((size_t)((D.d[0] + kT0 - 1) / kT0) > 65535 || (size_t)((D.d[1] + kT1 - 1) / kT1) > 65535 || n > 0x7fffffffull)
    refuse(fn, "shape " + triple(a.shape) + " is too large: at most 2^31 - 1 voxels");
  const bool conv = stage <= MCGPU_SEGMENT_TRAIN_STAGE_CONV_DGRAD;
  if (!a.in2 && stage != MCGPU_SEGMENT_TRAIN_STAGE_CONV_WGRAD) refuse(fn, "in2 is NULL");
  if (stage <= MCGPU_SEGMENT_TRAIN_STAGE_MAXPOOL_BACKWARD && (a.c1 < 1 || a.c1 > 65535)) refuse(fn, "c1 is " + std::to_string(a.c1) + ", expected 1..65535");
  if (conv && (a.c2 < 0 || a.c2 > 65535 || a.c_out < 1 || a.c_out > 65535))
    refuse(fn, "c2 is " + std::to_string(a.c2) + " and c_out " + std::to_string(a.c_out) + ", expected 0..65535 and 1..65535");
  if (stage == MCGPU_SEGMENT_TRAIN_STAGE_CONV_WGRAD && (!a.in3 || (a.c2 > 0 && !a.in2))) refuse(fn, "in2 or in3 is NULL");
  if (stage == MCGPU_SEGMENT_TRAIN_STAGE_CONV_DGRAD && a.c2 > 0 && !a.out2) refuse(fn, "out2 is NULL");
  if (stage == MCGPU_SEGMENT_TRAIN_STAGE_LOSS && (!a.values || a.n < 1 || a.n > 65535)) refuse(fn, "values is NULL, or n is not 1..65535");
  const auto t0 = std::chrono::steady_clock::now();
  TrainRunner R;
  R.init(a.device, std::max(std::max(a.c1, a.c_out), 1));
  switch (stage) {
    case MCGPU_SEGMENT_TRAIN_STAGE_CONV_WGRAD:
      stage_wgrad(R, a, D);
      break;
    case MCGPU_SEGMENT_TRAIN_STAGE_CONV_DGRAD: {
      const Dims E = a.upsample ? D.halved_up() : D;
      size_t cursor = 0;
      ConvLayer l = conv_layer(a.c1 + a.c2, a.c_out, cursor);
      Dgrad d(l, a.c1);
      const float* d_dy = R.upload(a.in, (size_t)a.c_out * n);
      const float* d_w = R.upload(a.in2, (size_t)a.c_out * l.c_in * kTaps);
      const float* d_zero = R.alloc((size_t)l.c_in + 1);
      d.first.wpack = R.alloc(d.first.pack_floats());
      d.first.bias = d_zero;
      d.second.wpack = R.alloc(d.second.pack_floats());
      d.second.bias = d_zero;
      float* d_ext = R.alloc((size_t)std::max(a.c2, 1) * n);
      float* d_o1 = R.alloc((size_t)a.c1 * n);
      float* d_o2 = R.alloc((size_t)std::max(a.c2, 1) * E.voxels());
      d.pack(l, d_w);
      Stage st(R.dev, R.rep.ms_dgrad);
      launch_dgrad(d, d_dy, D, d_ext, a.upsample, d_o1, d_o2);
      st.done();
      HIP_TRY(hipMemcpy(a.out, d_o1, (size_t)a.c1 * n * 4, hipMemcpyDeviceToHost));
      if (a.c2) HIP_TRY(hipMemcpy(a.out2, d_o2, (size_t)a.c2 * E.voxels() * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SEGMENT_TRAIN_STAGE_MAXPOOL_BACKWARD:
      stage_maxpool_backward(R, a, D, a.in3);
      break;
    default: {
      const size_t B = (size_t)a.n, m = (size_t)kClasses * n;
      const float* d_z = R.upload(a.in, B * m);
      const float* d_t = R.upload(a.in2, B * m);
      float* d_g = R.alloc(B * m);
      double* d_dice = (double*)R.alloc_bytes((size_t)kMaxSegments * kDiceSums * kClasses * sizeof(double), true);
      double* d_f = (double*)R.alloc_bytes(B * kClasses * sizeof(double), true);
      double2* d_coef = (double2*)R.alloc_bytes((size_t)kClasses * sizeof(double2), true);
      Stage st(R.dev, R.rep.ms_forward);
      for (size_t p = 0; p < B; ++p) {
        launch_dice(d_z + p * m, d_t + p * m, n, d_dice, d_f + p * kClasses, d_coef);
        hipLaunchKernelGGL(head_grad_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_z + p * m, d_t + p * m, d_coef, n, 1.0 / ((double)kClasses * (double)B),
                           d_g + p * m);
      }
      st.done();
      HIP_TRY(hipMemcpy(a.values + 1, d_f, B * kClasses * sizeof(double), hipMemcpyDeviceToHost));
      fill_losses(R.rep, (int)B, a.values + 1);
      a.values[0] = R.rep.loss;
      HIP_TRY(hipMemcpy(a.out, d_g, B * m * 4, hipMemcpyDeviceToHost));
    }
  }
  finish_report(R, t0, report);
  return 0;
  ABI_END
}
