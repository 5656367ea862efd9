// speedup_train.hip -- training of the speed-up network on the device: the backward half of speedup_net.hip, the two losses of the
// reference's trainer (cbctmc/speedup/trainer.py: MCSpeedUpTrainer._train_or_test_on_batch) and Adam, in float32.
//
// The rule.  A batch is B samples (low_photon lp, forward_projection or none, high_photon t), each [nv][nu]; N = B nv nu.
//   Forward: exactly mcgpu_speedup_run's (speedup_net.hip's header): preprocessing, mean net, m = relu(lp + 10 tanh(net_m)),
//     variance net on m, v = m 0.1 sigmoid(s) + 1e-6.  Instance norm keeps samples independent: every sample runs alone, the batch
//     gradient is the sum of the per-sample gradients added in sample order (float32), and the losses are sums over samples in
//     float64 divided by N.  No atomics anywhere: the same call gives the same bytes.  1 / N = 1 / (nv nu) x 1 / B is applied in two
//     places: a sample's backward pass runs on the gradient of its own mean loss, 1 / (nv nu), so that it is the same bytes in any
//     batch, and 1 / B multiplies the sample's float64-folded weight gradient where it is rounded to float32 and added.
//   Phase mean:      loss = mean |m - t|;  dL/dm = sign(m - t) / N (sign 0 = 0);  dL/dnet_m = dL/dm [m > 0] 10 (1 - tanh^2(net_m)).
//                    Only the mean net's weights get gradients.
//   Phase variance:  loss = mean 0.5 (log v' + (m - t)^2 / v'), v' = max(v, 1e-6);  dL/dv = 0.5 (1 / v' - (m - t)^2 / v'^2) / N where
//                    v > 1e-6, else 0;  dL/ds = dL/dv m 0.1 sigmoid(s) (1 - sigmoid(s)).  The mean net is frozen and no gradient is
//                    taken through m (the reference's second stage); only the variance net's weights get gradients.
//     The reference's joint stage (n_pretrain_steps = None) is not built.  The reference trains under float16 autocast with a
//     gradient scaler; here everything is float32 and nothing is scaled.
//   Backward of one FlexUNet: NetPass::forward walked in reverse.
//     LeakyReLU + instance norm:  d xh = dy (xh > 0 ? 1 : 0.01);  dx = rstd (d xh - mean(d xh) - xh mean(d xh xh)).  The two means are
//       float64 sums over stats_kernel's segments and a 256-wide tree; dx is computed in float64 and rounded once.  The forward pass
//       normalises in place, so the pass keeps y and every layer's own sums (mean, rstd); xh is recovered from y through the inverse
//       of the LeakyReLU (y > 0 ? y : y / 0.01f, in float64): within half a spacing of the xh that the forward rounded, against
//       keeping a second copy of every normed tensor (profiles/speedup_train.md has the measured gradient error of both).
//     Convolution, weights:  dW[co][ci][tap] = sum over pixels of dY[co][y][x] X~[ci][y + dy - 1][x + dx - 1], X~ what the forward
//       stages (clamped coordinates, two concatenated sources, the second through >> 1).
//     Convolution, bias:  db[co] = sum dY for init_conv and final_conv (float64 sums, rounded once); defined as exactly 0 for a
//       convolution that feeds an instance norm (mathematically 0; autograd gives rounding noise there) -- those biases never move.
//     Convolution, input:  the adjoint of clamp-then-convolve: the zero-padded correlation of dY with the weights transposed in
//       (co, ci) and flipped in the taps, on rows -1 .. H and columns -1 .. W; row -1 folds into row 0, row H into row H - 1, columns
//       alike (corners twice); channels of the first source go to the skip's gradient, channels of the second are summed over each
//       2 x 2 block into the half-size gradient (the adjoint of the nearest upsample).  init_conv needs none.
//     Max-pool:  the gradient goes to the first maximal element of the window in the order (0,0), (0,1), (1,0), (1,1), recomputed
//       from the saved input, and is added to what the decoder path left in the skip's gradient.
//   Adam (no weight decay):  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  w <- w - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) +
//     1e-8), per element in float64 from the float32 state, each result rounded once; t counts the updates of the phase's net; lr <- lr
//     gamma after every update.  A gradient of 0 on zero moments leaves w, m and v as they are.
//
// The kernels.
//   conv_wgrad_mfma_kernel: a GEMM on v_mfma_f32_32x32x2_f32 with M = C_out, N = C_in per tap, K = pixels.  A workgroup of 4 waves owns
//     32 output channels x 32 input channels x 9 taps and a range of pixel tiles (4 rows x 32 columns; a wave owns one row).  Per tile
//     the 6 x 34 halo of the 32 input channels is staged in LDS exactly as the forward stages it (the concatenated or upsampled input
//     never exists in memory) beside the 4 x 32 tile of dY, zero outside the image; channel strides are odd (205, 129), so that the 32
//     channels a wave reads at one pixel lie in 32 banks.  One MFMA k-step is two neighbouring pixels of a row; the nine taps are nine
//     accumulators fed from one dY value and nine shifted reads.  K is split across workgroups and waves into float32 partials
//     [partial][C_out][C_in][9]; wgrad_fold_kernel adds them in float64 in the order of the partials and rounds once.
//   Input gradient: conv3x3_mfma_kernel<NB, true> of speedup_conv.inc -- the forward's implicit GEMM with zero-filled staging --
//     with a second packing of the weights (pack_dgrad_weights_kernel: transposed, taps flipped) into an extended
//     [C_in][H + 2][W + 2] buffer, then dgrad_fold_kernel (fold of the border, split into the two sources, 2 x 2 sums; float64, rounded
//     once).
//   maxpool_backward_kernel, metrics_kernel (the four float64 sums of a sample: |m - t|, the Gaussian term, (lp - t)^2, (m - t)^2),
//     l1_grad_kernel, nll_grad_kernel; from unet_train_common.inc, shared with segment_train.hip: norm_backward_stats_kernel +
//     norm_backward_kernel, wgrad_fold_kernel, bias_grad_kernel, adam_kernel.
// The weights, both moments, both packings and all buffers of a pass live on the device between steps behind a handle; both packings
// of the phase's net are redone on the device after each update.
#include <chrono>
#include <memory>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

constexpr int kTaps = 9;
#include "unet_common.inc"
#include "speedup_conv.inc"
#include "unet_train_common.inc"

// ------------------------------------------------------------------------------------------------ convolution, weight gradient
constexpr int kWgH = 4;                                      // rows of a pixel tile: one per wave
constexpr int kWgHalo = (kWgH + 2) * kHaloW;                 // 204
constexpr int kWgXStride = kWgHalo + 1, kWgYStride = kWgH * kTileW + 1;  // odd: 32 channels at one pixel lie in 32 banks
constexpr int kWgTarget = 500;                               // workgroups to aim for when K is split

struct WgradArgs {
  const float* src1;  // [c1][H][W]
  const float* src2;  // [c2][H2][W2] or nullptr
  int c1, c2, H, W, H2, W2, ups;
  const float* dy;    // [c_out][H][W]
  int c_out;
  float* part;        // [4 splits][c_out][c1 + c2][9]
  int tiles_x, n_tiles, tiles_per_split;
};

__global__ __launch_bounds__(256) void conv_wgrad_mfma_kernel(WgradArgs a) {
  __shared__ float s_x[32 * kWgXStride];
  __shared__ float s_dy[32 * kWgYStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int split = blockIdx.x, cob = blockIdx.y, cib = blockIdx.z;
  const int c_in = a.c1 + a.c2;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* pa = s_dy + col * kWgYStride + wave * kTileW + h;  // A[co = col][pixel 2 k + h] of the wave's row
  const float* pb = s_x + col * kWgXStride + wave * kHaloW + h;   // B[pixel][ci = col]
  const int t_end = min((split + 1) * a.tiles_per_split, a.n_tiles);
  for (int t = split * a.tiles_per_split; t < t_end; ++t) {
    const int x0 = (t % a.tiles_x) * kTileW, y0 = (t / a.tiles_x) * kWgH;
    __syncthreads();  // the reads of the tile before
    for (int e = tid; e < 32 * kWgHalo; e += 256) {
      const int c = e / kWgHalo, r = e - c * kWgHalo, yy = r / kHaloW, xx = r - yy * kHaloW;
      const int gc = cib * 32 + c;
      const int y = min(max(y0 + yy - 1, 0), a.H - 1), x = min(max(x0 + xx - 1, 0), a.W - 1);  // replicate padding, as the forward
      float v = 0.f;
      if (gc < a.c1) v = a.src1[((size_t)gc * a.H + y) * a.W + x];
      else if (gc < c_in) v = a.src2[((size_t)(gc - a.c1) * a.H2 + (y >> a.ups)) * a.W2 + (x >> a.ups)];
      s_x[c * kWgXStride + r] = v;
    }
    for (int e = tid; e < 32 * kWgH * kTileW; e += 256) {
      const int c = e / (kWgH * kTileW), r = e - c * (kWgH * kTileW), yy = r / kTileW, xx = r - yy * kTileW;
      const int co = cob * 32 + c, y = y0 + yy, x = x0 + xx;
      s_dy[c * kWgYStride + r] = (co < a.c_out && y < a.H && x < a.W) ? a.dy[((size_t)co * a.H + y) * a.W + x] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kTileW / 2; ++k) {
      const float av = pa[2 * k];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float bv = pb[(tap / 3) * kHaloW + 2 * k + tap % 3];
        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tap], 0, 0, 0);
      }
    }
  }
  const int ci = cib * 32 + col;
  if (ci >= c_in) return;
  float* out = a.part + (size_t)(split * 4 + wave) * ((size_t)a.c_out * c_in * 9);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = cob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;  // the 32x32 C/D map: row of register r in lane half h
    if (co < a.c_out) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) out[((size_t)co * c_in + ci) * 9 + tap] = acc[tap][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------- convolution, input gradient
// The forward packing (unet_common.inc: pack_weights_kernel) of W'[ci][co][tap] = W[co][ci][8 - tap]: the GEMM's input channels
// are the layer's output channels
__global__ __launch_bounds__(256) void pack_dgrad_weights_kernel(const float* w, float* wpack, int c_in, int c_out, int n_chunks, int ncol, size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int out_local = (int)(e % ncol);
  size_t r = e / ncol;
  const int kk = (int)(r % kKK);
  r /= kKK;
  const int ch = (int)(r % n_chunks), cb = (int)(r / n_chunks);
  const int hh = kk & 1, tap = (kk >> 1) % 9, cp = (kk >> 1) / 9;
  const int co = ch * kCK + cp * 2 + hh, ci = cb * ncol + out_local;  // of the layer
  wpack[e] = (ci < c_in && co < c_out) ? w[((size_t)co * c_in + ci) * 9 + (8 - tap)] : 0.f;
}

// one pixel of the folded gradient of channel image e [(H + 2)][(W + 2)]: what the clamp sent to (y, x), added in float64
__device__ double folded(const float* e, int H, int W, int y, int x) {
  const int ya = y == 0 ? 0 : y + 1, yb = y == H - 1 ? H + 1 : y + 1;
  const int xa = x == 0 ? 0 : x + 1, xb = x == W - 1 ? W + 1 : x + 1;
  double s = 0.0;
  for (int yy = ya; yy <= yb; ++yy)
    for (int xx = xa; xx <= xb; ++xx) s += (double)e[(size_t)yy * (W + 2) + xx];
  return s;
}

// out1 [c1][H][W] = fold(ext channels 0 .. c1); out2 [c2][H2][W2] = fold(ext channels c1 ..), summed over 2 x 2 blocks when ups
__global__ __launch_bounds__(256) void dgrad_fold_kernel(const float* ext, int c1, int c2, int H, int W, int H2, int W2, int ups, float* out1, float* out2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n1 = (size_t)c1 * H * W, n2 = (size_t)c2 * H2 * W2, plane = (size_t)(H + 2) * (W + 2);
  if (i < n1) {
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((size_t)W * H));
    out1[i] = (float)folded(ext + (size_t)c * plane, H, W, y, x);
  } else if (i < n1 + n2) {
    const size_t j = i - n1;
    const int x2 = (int)(j % W2), y2 = (int)((j / W2) % H2), c = (int)(j / ((size_t)W2 * H2));
    const float* e = ext + (size_t)(c1 + c) * plane;
    double s = 0.0;
    if (ups) {
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx)
          if (2 * y2 + dy < H && 2 * x2 + dx < W) s += folded(e, H, W, 2 * y2 + dy, 2 * x2 + dx);
    } else {
      s = folded(e, H, W, y2, x2);
    }
    out2[j] = (float)s;
  }
}

// ------------------------------------------------------------------------------------------------------------ small kernels
// dx[first maximum of the window] += dy
__global__ __launch_bounds__(256) void maxpool_backward_kernel(const float* x, const float* dy, float* dx, int C, int H, int W) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)C * Ho * Wo) return;
  const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho), c = (int)(i / ((size_t)Wo * Ho));
  const size_t base = ((size_t)c * H + 2 * yo) * W + 2 * xo;
  const float* p = x + base;
  const float m = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
  const size_t at = p[0] == m ? 0 : p[1] == m ? 1 : p[W] == m ? (size_t)W : (size_t)W + 1;
  dx[base + at] += dy[i];
}

using Sums4 = Sums<4>;

// part[s] = float64 sums over segment s of |m - t|, 0.5 (log v' + (m - t)^2 / v'), (lp - t)^2, (m - t)^2
__global__ __launch_bounds__(256) void metrics_kernel(const float* lp, const float* m, const float* v, const float* t, size_t hw, int S, Sums4* part) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const Segment g = segment_of(hw, S, s);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t i = g.lo + tid; i < g.hi; i += 256) {
    const double d = (double)m[i] - (double)t[i], e = (double)lp[i] - (double)t[i];
    a[0] += fabs(d);
    if (v) {
      const double vv = fmax((double)v[i], 1e-6);
      a[1] += 0.5 * (log(vv) + d * d / vv);
    }
    a[2] += e * e;
    a[3] += d * d;
  }
  const Sums4 total = block_tree(Sums4{{a[0], a[1], a[2], a[3]}});
  if (tid == 0) part[s] = total;
}

// dL/dnet of the L1 loss through m = relu(lp + 10 tanh(net)); inv_n = 1 / N
__global__ __launch_bounds__(256) void l1_grad_kernel(const float* m, const float* t, const float* net, float* g, size_t hw, double inv_n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const double d = (double)m[i] - (double)t[i], th = tanh((double)net[i]);
  const double sign = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
  g[i] = m[i] > 0.f ? (float)(sign * inv_n * 10.0 * (1.0 - th * th)) : 0.f;
}

// dL/ds of the Gaussian loss through v = m 0.1 sigmoid(s) + 1e-6, m held fixed
__global__ __launch_bounds__(256) void nll_grad_kernel(const float* m, const float* v, const float* t, const float* s, float* g, size_t hw, double inv_n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  float out = 0.f;
  if ((double)v[i] > 1e-6) {
    const double d = (double)m[i] - (double)t[i], vv = (double)v[i], sg = 1.0 / (1.0 + exp(-(double)s[i]));
    out = (float)(0.5 * (1.0 / vv - d * d / (vv * vv)) * inv_n * (double)m[i] * 0.1 * sg * (1.0 - sg));
  }
  g[i] = out;
}

// -------------------------------------------------------------------------------------------------------------------- host
using Report = mcgpu_speedup_train_report;

// how K of a layer's weight gradient is split: tiles of 4 x 32 pixels per workgroup, 4 partials (waves) per workgroup
struct WgradPlan {
  int tiles_x, n_tiles, tiles_per_split, splits;
  int partials() const { return 4 * splits; }
};
WgradPlan wgrad_plan(int c_in, int c_out, const Dims& D) {
  WgradPlan p;
  p.tiles_x = (D.W + kTileW - 1) / kTileW;
  p.n_tiles = p.tiles_x * ((D.H + kWgH - 1) / kWgH);
  const int blocks = ((c_out + 31) / 32) * ((c_in + 31) / 32);
  const int want = std::min(p.n_tiles, std::max(1, (kWgTarget + blocks - 1) / blocks));
  p.tiles_per_split = (p.n_tiles + want - 1) / want;
  p.splits = (p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}
size_t wgrad_part_floats(int c_in, int c_out, const Dims& D) { return (size_t)wgrad_plan(c_in, c_out, D).partials() * c_out * c_in * 9; }

// grad_w [c_out][c_in][9] += scale dW; grad_b [c_out] += scale db when grad_b
void launch_wgrad(RunnerBase<Report>& R, int c_out, const float* src1, int c1, const float* src2, int c2, int ups, const Dims& D, const float* dy, float* part,
                  float* grad_w, float* grad_b, double scale) {
  const Dims E = ups ? D.halved_up() : D;
  const WgradPlan p = wgrad_plan(c1 + c2, c_out, D);
  WgradArgs a;
  a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = c2; a.H = D.H; a.W = D.W; a.H2 = E.H; a.W2 = E.W; a.ups = ups ? 1 : 0;
  a.dy = dy; a.c_out = c_out; a.part = part; a.tiles_x = p.tiles_x; a.n_tiles = p.n_tiles; a.tiles_per_split = p.tiles_per_split;
  hipLaunchKernelGGL(conv_wgrad_mfma_kernel, dim3((unsigned)p.splits, (unsigned)((c_out + 31) / 32), (unsigned)((c1 + c2 + 31) / 32)), dim3(256), 0, nullptr, a);
  launch_wgrad_fold(part, p.partials(), (size_t)c_out * (c1 + c2) * 9, grad_w, dy, c_out, D.voxels(), R.d_part, grad_b, scale);
}

// The input-gradient GEMM of a layer: its input channels are the layer's output channels.  c1: the channels of the layer's first source
struct Dgrad {
  ConvLayer g;  // c_out 0: none
  int c1 = 0;
  Dgrad() = default;
  Dgrad(const ConvLayer& l, int c1_) : c1(c1_) {
    g.c_in = l.c_out;
    g.c_out = l.c_in;
    g.nb = blocks_per_workgroup(g.c_out);
    g.n_chunks = (g.c_in + kCK - 1) / kCK;
  }
  template <class F>
  void each(F f) { if (g.c_out) f(g); }
  void pack(const ConvLayer& l, const float* d_w) const {
    const size_t total = g.pack_floats();
    if (total) hipLaunchKernelGGL(pack_dgrad_weights_kernel, dim3(blocks_of(total)), dim3(256), 0, nullptr, d_w, g.wpack, l.c_in, l.c_out, g.n_chunks, 32 * g.nb, total);
  }
};
size_t dgrad_ext_floats(const ConvLayer& l, int, const Dims& D) { return (size_t)l.c_in * (D.H + 2) * (D.W + 2); }

// out1 [c1][H][W], out2 [c_in - c1][..] = the gradient of the layer's two sources; d: packed, its bias zeros; ext: dgrad_ext_floats
void launch_dgrad(const Dgrad& dg, const float* dy, const Dims& D, float* ext, int ups, float* out1, float* out2) {
  const ConvLayer& d = dg.g;
  const int c1 = dg.c1;
  const Dims E = ups ? D.halved_up() : D;
  ConvArgs a;
  a.src1 = dy; a.src2 = nullptr; a.c1 = d.c_in; a.c2 = 0; a.H = D.H + 2; a.W = D.W + 2; a.H2 = D.H; a.W2 = D.W; a.ups = 0;
  a.wpack = d.wpack; a.bias = d.bias; a.out = ext; a.c_out = d.c_out; a.n_chunks = d.n_chunks;
  const dim3 grid((unsigned)((a.W + kTileW - 1) / kTileW), (unsigned)((a.H + kTileH - 1) / kTileH), (unsigned)((d.c_out + 32 * d.nb - 1) / (32 * d.nb)));
  if (d.nb == 2) hipLaunchKernelGGL((conv3x3_mfma_kernel<2, true>), grid, dim3(256), 0, nullptr, a);
  else hipLaunchKernelGGL((conv3x3_mfma_kernel<1, true>), grid, dim3(256), 0, nullptr, a);
  const int c2 = d.c_out - c1;
  const size_t n = (size_t)c1 * D.voxels() + (size_t)c2 * E.voxels();
  hipLaunchKernelGGL(dgrad_fold_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, ext, c1, c2, D.H, D.W, E.H, E.W, ups ? 1 : 0, out1, out2);
}

void launch_maxpool_backward(const float* x, const float* dy, float* dx, int C, const Dims& D) {
  const size_t n = (size_t)C * D.shifted(1).voxels();
  if (n) hipLaunchKernelGGL(maxpool_backward_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, dy, dx, C, D.H, D.W);
}

#include "unet_train_host.inc"

// the preprocessing of the mean net's second channel needs the sums of two images
struct SpeedupRunner : TrainRunner {
  double2* d_part2 = nullptr;  // the second image of the preprocessing

  void init(int device, int channels) {
    TrainRunner::init(device, channels);
    d_part2 = (double2*)alloc_bytes(kMaxSegments * sizeof(double2), true);
  }
  void preprocess(const float* lp, const float* fp, float* out, size_t hw) {
    stats(lp, 1, hw, d_part);
    stats(fp, 1, hw, d_part2);
    hipLaunchKernelGGL(preprocess_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, fp, out, hw, segments_of(hw), d_part, d_part2);
  }
};

// the layers of one net, each with the variant of the forward convolution that speedup_net.hip runs it with
NetLayers train_layers(const NetShape& s, size_t& cursor) {
  NetLayers net = layers_of(s, cursor);
  net.each([](ConvLayer& l) { l.nb = blocks_per_workgroup(l.c_out); });
  return net;
}

}  // namespace

struct mcgpu_speedup_trainer {
  mcgpu_speedup_train_options o;
  SpeedupRunner R;
  TrainCore core;
  Dims P;
  size_t hw = 0;
  float *d_x = nullptr, *d_fp = nullptr, *d_t = nullptr, *d_mean = nullptr, *d_var = nullptr;
  Sums4* d_sums = nullptr;
  std::unique_ptr<TrainNet> mean_net, var_net;
  unsigned long long step_mean = 0, step_var = 0;
  double lr = 0.0;
};

namespace {

using Trainer = mcgpu_speedup_trainer;

void check_create(const char* fn, const mcgpu_speedup_train_options& o) {
  if (o.nu < 1 || o.nv < 1 || o.max_batch < 1) refuse(fn, "nu, nv and max_batch must be >= 1");
  if ((unsigned long long)o.nu * (unsigned long long)o.nv > 0x7fffffffull) refuse(fn, "nu x nv must be below 2^31");
  if (!o.weights) refuse(fn, "weights is NULL");
  const NetShape m{o.mean_in_channels, o.mean_levels, o.mean_filter_base}, v{o.var_in_channels, o.var_levels, o.var_filter_base};
  if (!shape_ok(m) || !shape_ok(v) || m.in_channels > 2 || v.in_channels != 1)
    refuse(fn, "bad architecture: mean_in_channels 1 or 2, var_in_channels 1, levels 1..8, filter_base 1..1024");
  size_t expect = 0;
  layers_of(m, expect);
  layers_of(v, expect);
  if (o.n_weights != expect)
    refuse(fn, "n_weights is " + std::to_string(o.n_weights) + " but the architecture has " + std::to_string(expect) + " values");
  const int deep = std::max(m.levels, v.levels);
  if (o.nu % (1 << deep) || o.nv % (1 << deep))
    refuse(fn, "nu and nv must be divisible by " + std::to_string(1 << deep) + " (2^levels): " + std::to_string(o.nu) + " x " + std::to_string(o.nv));
  if ((size_t)(o.nu >> deep) * (o.nv >> deep) < 2)
    refuse(fn, "the bottleneck of a " + std::to_string(o.nu) + " x " + std::to_string(o.nv) + " image has fewer than 2 pixels: instance norm is undefined");
  if (!(o.lr > 0.0) || !(o.gamma > 0.0 && o.gamma <= 1.0)) refuse(fn, "lr must be > 0 and gamma in (0, 1]");
  if (!(o.beta1 >= 0.0 && o.beta1 < 1.0) || !(o.beta2 >= 0.0 && o.beta2 < 1.0)) refuse(fn, "beta1 and beta2 must be in [0, 1)");
}

void check_batch(const char* fn, const Trainer* T, int phase, int n, const float* lp, const float* fp, const float* t, bool need_target) {
  if (!T) refuse(fn, "handle is NULL");
  if (phase != MCGPU_SPEEDUP_PHASE_MEAN && phase != MCGPU_SPEEDUP_PHASE_VARIANCE) refuse(fn, "unknown phase " + std::to_string(phase));
  if (n < 1 || n > T->o.max_batch) refuse(fn, "n is " + std::to_string(n) + " but the trainer was created for 1.." + std::to_string(T->o.max_batch));
  if (!lp) refuse(fn, "low_photon is NULL");
  if (need_target && !t) refuse(fn, "high_photon is NULL");
  if (T->o.mean_in_channels == 2 && !fp) refuse(fn, "forward_projection is NULL but the mean net has 2 input channels");
  if (T->o.mean_in_channels == 1 && fp) refuse(fn, "the mean net has 1 input channel: forward_projection must be NULL");
  if (fp) {
    const int p = constant_slice(fp, n, T->hw);
    if (p >= 0) refuse(fn, "forward_projection slice " + std::to_string(p) + " has zero variance: it cannot be matched to the low-photon projection");
  }
}

// mean and variance of sample p on the device (d_x, d_mean, d_var), every layer's output and sums kept for the backward
void forward_sample(Trainer& T, const float* lp, const float* fp, int p) {
  SpeedupRunner& R = T.R;
  const size_t hw = T.hw;
  HIP_TRY(hipMemcpy(T.d_x, lp + (size_t)p * hw, hw * 4, hipMemcpyHostToDevice));
  if (fp) {
    HIP_TRY(hipMemcpy(T.d_fp, fp + (size_t)p * hw, hw * 4, hipMemcpyHostToDevice));
    R.preprocess(T.d_x, T.d_fp, T.d_x + hw, hw);
  }
  R.norm_parts = &T.mean_net->parts;
  R.norm_i = 0;
  const float* net_mean = T.mean_net->act->forward(T.d_x);
  hipLaunchKernelGGL(head_mean_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, T.d_x, net_mean, T.d_mean, hw);
  R.norm_parts = &T.var_net->parts;
  R.norm_i = 0;
  const float* net_var = T.var_net->act->forward(T.d_mean);
  hipLaunchKernelGGL(head_variance_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, T.d_mean, net_var, T.d_var, hw);
  R.norm_parts = nullptr;
}

struct BatchSums { double v[4] = {0.0, 0.0, 0.0, 0.0}; };

// forward of every sample, its sums, and (with `gradient`) its gradient of the phase's loss added to d_grad
void run_batch(Trainer& T, int phase, int n, const float* lp, const float* fp, const float* t, bool gradient, BatchSums& sums) {
  SpeedupRunner& R = T.R;
  const size_t hw = T.hw;
  const int S = segments_of(hw);
  // A sample's backward pass runs on the gradient of ITS mean loss (1 / (nv nu)) and is the same bytes in any batch; the share 1 / B
  // of the batch is applied where the sample's gradient is rounded to float32 and added to the batch's
  const double inv_hw = 1.0 / (double)hw, inv_b = 1.0 / (double)n;
  if (gradient) HIP_TRY(hipMemset(T.core.d_grad, 0, T.core.n_w * 4));
  std::vector<Sums4> host((size_t)S * n);
  for (int p = 0; p < n; ++p) {
    {
      Stage st(R.dev, R.rep.ms_forward);
      forward_sample(T, lp, fp, p);
      HIP_TRY(hipMemcpy(T.d_t, t + (size_t)p * hw, hw * 4, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(metrics_kernel, dim3((unsigned)S), dim3(256), 0, nullptr, T.d_x, T.d_mean, T.d_var, T.d_t, hw, S, T.d_sums + (size_t)p * S);
      st.done();
    }
    if (!gradient) continue;
    if (phase == MCGPU_SPEEDUP_PHASE_MEAN) {
      hipLaunchKernelGGL(l1_grad_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, T.d_mean, T.d_t, T.mean_net->act->out, T.mean_net->grad->out, hw, inv_hw);
      backward_sample(R, *T.mean_net, T.d_x, T.core, inv_b);
    } else {
      hipLaunchKernelGGL(nll_grad_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, T.d_mean, T.d_var, T.d_t, T.var_net->act->out, T.var_net->grad->out, hw,
                         inv_hw);
      backward_sample(R, *T.var_net, T.d_mean, T.core, inv_b);
    }
  }
  HIP_TRY(hipMemcpy(host.data(), T.d_sums, host.size() * sizeof(Sums4), hipMemcpyDeviceToHost));  // once per batch; waits for the device
  for (size_t s = 0; s < host.size(); ++s)  // samples in order, segments in order
    for (int k = 0; k < 4; ++k) sums.v[k] += host[s].v[k];
}

void fill_report(Trainer& T, int phase, int n, const BatchSums& s, const std::chrono::steady_clock::time_point& t0, Report* report) {
  const double N = (double)n * (double)T.hw;
  Report& r = T.R.rep;
  r.phase = phase;
  r.l1_loss = s.v[0] / N;
  r.gaussian_nll_loss = s.v[1] / N;
  r.loss = phase == MCGPU_SPEEDUP_PHASE_MEAN ? r.l1_loss : r.gaussian_nll_loss;
  r.psnr_before = 20.0 * std::log10(8.711442 / std::sqrt(s.v[2] / N));
  r.psnr_after = 20.0 * std::log10(8.711442 / std::sqrt(s.v[3] / N));
  r.step = T.step_mean + T.step_var;
  r.lr = T.lr;
  finish_report(T.R, t0, report);
}

}  // namespace

extern "C" int mcgpu_speedup_train_create(const mcgpu_speedup_train_options* caller_o, mcgpu_speedup_trainer** handle) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_create";
  if (!handle) refuse(fn, "handle is NULL");
  *handle = nullptr;
  std::unique_ptr<Trainer> T(new Trainer);
  mcgpu::read_options(fn, "mcgpu_speedup_train_options", caller_o, T->o);
  const mcgpu_speedup_train_options& o = T->o;
  check_create(fn, o);
  SpeedupRunner& R = T->R;
  R.dry = o.dry != 0;
  T->P = Dims{o.nv, o.nu};
  T->hw = T->P.voxels();
  T->lr = o.lr;
  const size_t hw = T->hw;
  const NetShape ms{o.mean_in_channels, o.mean_levels, o.mean_filter_base}, vs{o.var_in_channels, o.var_levels, o.var_filter_base};
  size_t cursor = 0;
  NetLayers mean_layers = train_layers(ms, cursor), var_layers = train_layers(vs, cursor);
  const int widest = std::max(mean_layers.widest(), var_layers.widest());
  R.init(o.device, widest);
  TrainCore& C = T->core;
  C.alloc(R, o.device, o.weights, (size_t)o.n_weights, widest);
  T->d_x = R.alloc(2 * hw);  // channel 0: the low-photon projection, channel 1: the matched forward projection
  T->d_fp = R.alloc(hw);
  T->d_t = R.alloc(hw);
  T->d_mean = R.alloc(hw);
  T->d_var = R.alloc(hw);
  T->d_sums = (Sums4*)R.alloc_bytes((size_t)o.max_batch * kMaxSegments * sizeof(Sums4), true);  // of every sample of a batch
  T->mean_net.reset(new TrainNet(std::move(mean_layers), R, T->P, C.d_w, C.d_zero));
  T->var_net.reset(new TrainNet(std::move(var_layers), R, T->P, C.d_w, C.d_zero));
  C.alloc_scratch(std::max(T->mean_net->part_floats, T->var_net->part_floats), std::max(T->mean_net->ext_floats, T->var_net->ext_floats));
  if (!R.dry) C.repack({T->mean_net.get(), T->var_net.get()});
  *handle = T.release();
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_step(mcgpu_speedup_trainer* T, int phase, int n, const float* low_photon, const float* forward_projection,
                                        const float* high_photon, int update, mcgpu_speedup_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_step";
  check_batch(fn, T, phase, n, low_photon, forward_projection, high_photon, true);
  mcgpu::check_report(fn, "report", "mcgpu_speedup_train_report", report);
  T->core.check_live(fn);
  const auto t0 = std::chrono::steady_clock::now();
  clear_times(T->R.rep);
  BatchSums sums;
  run_batch(*T, phase, n, low_photon, forward_projection, high_photon, update != 0, sums);
  if (update) {
    Stage st(T->R.dev, T->R.rep.ms_optimizer);
    TrainNet& N = phase == MCGPU_SPEEDUP_PHASE_MEAN ? *T->mean_net : *T->var_net;
    unsigned long long& t = phase == MCGPU_SPEEDUP_PHASE_MEAN ? T->step_mean : T->step_var;
    ++t;
    T->core.update(N, T->lr, T->o.beta1, T->o.beta2, t);
    st.done();
    T->lr *= T->o.gamma;
  }
  fill_report(*T, phase, n, sums, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_gradients(mcgpu_speedup_trainer* T, int phase, int n, const float* low_photon, const float* forward_projection,
                                             const float* high_photon, float* flat_gradient, mcgpu_speedup_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_gradients";
  check_batch(fn, T, phase, n, low_photon, forward_projection, high_photon, true);
  if (!flat_gradient) refuse(fn, "flat_gradient is NULL");
  mcgpu::check_report(fn, "report", "mcgpu_speedup_train_report", report);
  T->core.check_live(fn);
  const auto t0 = std::chrono::steady_clock::now();
  clear_times(T->R.rep);
  BatchSums sums;
  run_batch(*T, phase, n, low_photon, forward_projection, high_photon, true, sums);
  HIP_TRY(hipMemcpy(flat_gradient, T->core.d_grad, T->core.n_w * 4, hipMemcpyDeviceToHost));
  fill_report(*T, phase, n, sums, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_predict(mcgpu_speedup_trainer* T, int n, const float* low_photon, const float* forward_projection, float* mean,
                                           float* variance) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_predict";
  check_batch(fn, T, MCGPU_SPEEDUP_PHASE_MEAN, n, low_photon, forward_projection, nullptr, false);
  T->core.check_live(fn);
  for (int p = 0; p < n; ++p) {
    forward_sample(*T, low_photon, forward_projection, p);
    HIP_TRY(hipGetLastError());
    if (mean) HIP_TRY(hipMemcpy(mean + (size_t)p * T->hw, T->d_mean, T->hw * 4, hipMemcpyDeviceToHost));
    if (variance) HIP_TRY(hipMemcpy(variance + (size_t)p * T->hw, T->d_var, T->hw * 4, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_get_state(mcgpu_speedup_trainer* T, mcgpu_speedup_train_state* caller_s) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_get_state";
  if (!T) refuse(fn, "handle is NULL");
  mcgpu_speedup_train_state s;
  mcgpu::read_options(fn, "mcgpu_speedup_train_state", caller_s, s);
  T->core.check_state(fn, s);
  T->core.get_arrays(fn, s);
  s.n_weights = T->core.n_w;
  s.step_mean = T->step_mean;
  s.step_variance = T->step_var;
  s.lr = T->lr;
  s.planned_device_bytes = T->core.planned_bytes();
  mcgpu::write_report(caller_s, s);
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_set_state(mcgpu_speedup_trainer* T, const mcgpu_speedup_train_state* caller_s) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_set_state";
  if (!T) refuse(fn, "handle is NULL");
  mcgpu_speedup_train_state s;
  mcgpu::read_options(fn, "mcgpu_speedup_train_state", caller_s, s);
  T->core.check_state(fn, s);
  if (!(s.lr > 0.0)) refuse(fn, "lr must be > 0");
  T->core.set_arrays(fn, s, {T->mean_net.get(), T->var_net.get()});
  T->step_mean = s.step_mean;
  T->step_var = s.step_variance;
  T->lr = s.lr;
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_destroy(mcgpu_speedup_trainer* T) {
  ABI_BEGIN
  if (!T) return 0;
  if (!T->R.dry) (void)hipSetDevice(T->o.device);
  delete T;
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_train_stage(int stage, const mcgpu_speedup_train_stage_args* caller_a, mcgpu_speedup_train_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_train_stage";
  mcgpu_speedup_train_stage_args a;
  mcgpu::read_options(fn, "mcgpu_speedup_train_stage_args", caller_a, a);
  mcgpu::check_report(fn, "report", "mcgpu_speedup_train_report", report);
  if (stage < MCGPU_SPEEDUP_TRAIN_STAGE_CONV_WGRAD || stage > MCGPU_SPEEDUP_TRAIN_STAGE_ADAM) refuse(fn, "unknown stage " + std::to_string(stage));
  if (!a.in || !a.out) refuse(fn, "in or out is NULL");
  const bool conv = stage <= MCGPU_SPEEDUP_TRAIN_STAGE_CONV_DGRAD, loss = stage == MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_L1 || stage == MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_NLL;
  if (stage != MCGPU_SPEEDUP_TRAIN_STAGE_ADAM) {
    if (a.nu < 1 || a.nv < 1 || (unsigned long long)a.nu * (unsigned long long)a.nv > 0x7fffffffull) refuse(fn, "nu and nv must be >= 1 and nu x nv below 2^31");
    if (!a.in2 && stage != MCGPU_SPEEDUP_TRAIN_STAGE_CONV_WGRAD) refuse(fn, "in2 is NULL");
  }
  if (stage <= MCGPU_SPEEDUP_TRAIN_STAGE_MAXPOOL_BACKWARD && (a.c1 < 1 || a.c1 > 65536)) refuse(fn, "c1 must be 1..65536");
  if (conv && (a.c2 < 0 || a.c2 > 65536 || a.c_out < 1 || a.c_out > 65536)) refuse(fn, "c2 must be 0..65536 and c_out 1..65536");
  if (stage == MCGPU_SPEEDUP_TRAIN_STAGE_CONV_WGRAD && (!a.in3 || (a.c2 > 0 && !a.in2))) refuse(fn, "in2 or in3 is NULL");
  if (stage == MCGPU_SPEEDUP_TRAIN_STAGE_CONV_DGRAD && a.c2 > 0 && !a.out2) refuse(fn, "out2 is NULL");
  if (stage == MCGPU_SPEEDUP_TRAIN_STAGE_NORM_LRELU_BACKWARD && (size_t)a.nu * a.nv < 2) refuse(fn, "instance norm needs at least 2 pixels");
  if (loss && (!a.in3 || !a.values || a.n < 1)) refuse(fn, "in3 or values is NULL, or n is 0");
  if (stage == MCGPU_SPEEDUP_TRAIN_STAGE_ADAM) {
    if (!a.out2 || !a.out3 || a.n < 1 || a.step < 1) refuse(fn, "out2 or out3 is NULL, or n or step is 0");
    if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0)) refuse(fn, "beta1 and beta2 must be in [0, 1)");
  }
  const auto t0 = std::chrono::steady_clock::now();
  SpeedupRunner R;
  R.init(a.device, std::max(std::max(a.c1, a.c_out), 1));
  const Dims D{a.nv, a.nu};
  const size_t hw = D.voxels();
  switch (stage) {
    case MCGPU_SPEEDUP_TRAIN_STAGE_CONV_WGRAD:
      stage_wgrad(R, a, D);
      break;
    case MCGPU_SPEEDUP_TRAIN_STAGE_CONV_DGRAD: {
      const Dims E = a.upsample ? D.halved_up() : D;
      size_t cursor = 0;
      ConvLayer l = conv_layer(a.c1 + a.c2, a.c_out, cursor);
      Dgrad d(l, a.c1);
      const float* d_dy = R.upload(a.in, (size_t)a.c_out * hw);
      const float* d_w = R.upload(a.in2, (size_t)a.c_out * l.c_in * 9);
      d.g.wpack = R.alloc(d.g.pack_floats());
      d.g.bias = R.alloc((size_t)d.g.c_out);
      float* d_ext = R.alloc(dgrad_ext_floats(l, a.c1, D));
      float* d_o1 = R.alloc((size_t)a.c1 * hw);
      float* d_o2 = R.alloc((size_t)std::max(a.c2, 1) * E.voxels());
      d.pack(l, d_w);
      Stage st(R.dev, R.rep.ms_dgrad);
      launch_dgrad(d, d_dy, D, d_ext, a.upsample, d_o1, d_o2);
      st.done();
      HIP_TRY(hipMemcpy(a.out, d_o1, (size_t)a.c1 * hw * 4, hipMemcpyDeviceToHost));
      if (a.c2) HIP_TRY(hipMemcpy(a.out2, d_o2, (size_t)a.c2 * E.voxels() * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SPEEDUP_TRAIN_STAGE_NORM_LRELU_BACKWARD: {
      const float* d_x = R.upload(a.in, (size_t)a.c1 * hw);
      float* d_dy = R.upload(a.in2, (size_t)a.c1 * hw);
      float* d_y = R.alloc((size_t)a.c1 * hw);
      double2* d_bpart = (double2*)R.alloc_bytes((size_t)a.c1 * kMaxSegments * sizeof(double2), true);
      R.norm_lrelu(d_x, d_y, a.c1, hw);
      Stage st(R.dev, R.rep.ms_norm);
      launch_norm_backward(d_y, d_dy, a.c1, hw, R.d_part, d_bpart);
      st.done();
      HIP_TRY(hipMemcpy(a.out, d_dy, (size_t)a.c1 * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SPEEDUP_TRAIN_STAGE_MAXPOOL_BACKWARD:
      stage_maxpool_backward(R, a, D, nullptr);
      break;
    case MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_L1:
    case MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_NLL: {
      const bool l1 = stage == MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_L1;
      const size_t n = (size_t)a.n;
      const float* d_a = R.upload(a.in, n * hw);   // low_photon | mean
      const float* d_s = R.upload(a.in2, n * hw);  // the net's output
      const float* d_t = R.upload(a.in3, n * hw);
      float* d_head = R.alloc(n * hw);
      float* d_g = R.alloc(n * hw);
      Sums4* d_sums = (Sums4*)R.alloc_bytes(kMaxSegments * sizeof(Sums4), true);
      const int S = segments_of(hw);
      const double inv_n = 1.0 / ((double)n * (double)hw);
      std::vector<Sums4> host(S);
      double sum = 0.0;
      Stage st(R.dev, R.rep.ms_forward);
      for (size_t p = 0; p < n; ++p) {
        const size_t o = p * hw;
        if (l1) {
          hipLaunchKernelGGL(head_mean_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_a + o, d_s + o, d_head + o, hw);
          hipLaunchKernelGGL(metrics_kernel, dim3((unsigned)S), dim3(256), 0, nullptr, d_a + o, d_head + o, (const float*)nullptr, d_t + o, hw, S, d_sums);
          hipLaunchKernelGGL(l1_grad_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_head + o, d_t + o, d_s + o, d_g + o, hw, inv_n);
        } else {
          hipLaunchKernelGGL(head_variance_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_a + o, d_s + o, d_head + o, hw);
          hipLaunchKernelGGL(metrics_kernel, dim3((unsigned)S), dim3(256), 0, nullptr, d_a + o, d_a + o, d_head + o, d_t + o, hw, S, d_sums);
          hipLaunchKernelGGL(nll_grad_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_a + o, d_head + o, d_t + o, d_s + o, d_g + o, hw, inv_n);
        }
        HIP_TRY(hipMemcpy(host.data(), d_sums, S * sizeof(Sums4), hipMemcpyDeviceToHost));
        for (int s = 0; s < S; ++s) sum += host[s].v[l1 ? 0 : 1];
      }
      st.done();
      a.values[0] = sum * inv_n;
      HIP_TRY(hipMemcpy(a.out, d_g, n * hw * 4, hipMemcpyDeviceToHost));
      if (a.out2) HIP_TRY(hipMemcpy(a.out2, d_head, n * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    default: {
      const size_t n = (size_t)a.n;
      const float* d_g = R.upload(a.in, n);
      float* d_w = R.upload(a.out, n);
      float* d_m1 = R.upload(a.out2, n);
      float* d_m2 = R.upload(a.out3, n);
      Stage st(R.dev, R.rep.ms_optimizer);
      launch_adam(d_w, d_g, d_m1, d_m2, n, a.lr, a.beta1, a.beta2, a.step);
      st.done();
      HIP_TRY(hipMemcpy(a.out, d_w, n * 4, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(a.out2, d_m1, n * 4, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(a.out3, d_m2, n * 4, hipMemcpyDeviceToHost));
    }
  }
  finish_report(R, t0, report);
  return 0;
  ABI_END
}
