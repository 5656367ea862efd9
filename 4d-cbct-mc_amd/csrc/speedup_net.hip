// speedup_net.hip -- the reference's speed-up network (cbctmc/speedup: MCSpeedUpUNet behind MCSpeedup), inferred in float32.
//
// The network.  FlexUNet(C, L levels, base F), every convolution 3 x 3 with replicate padding and bias:
//   skip_0 = init_conv(x)                                                   C -> F, full size, no norm
//   skip_{i+1} = enc_i(skip_i), i = 0 .. L-1:  max-pool 2 x 2, then twice [conv -> instance norm -> LeakyReLU(0.01)] to F 2^i
//   dec_i, i = L-1 .. 0:  cat([skip_i, nearest-upsample x 2 of the running tensor]), then twice [conv -> norm -> LeakyReLU] to F 2^i
//   final_conv                                                              F -> 1
// Instance norm: per channel over H x W, biased variance, eps 1e-5, no affine parameters.
//   x = cat(low_photon, fp'),  fp' = (fp - mean(fp)) / std(fp) * std(low_photon) + mean(low_photon)   (unbiased std, per projection)
//   mean = relu(low_photon + 10 tanh(mean_net(x)))              mean_net = FlexUNet(2, 4, 64)
//   variance = mean * 0.10 sigmoid(var_net(mean)) + 1e-6        var_net = FlexUNet(1, 2, 16)
//   sample = mean + sqrt(variance) z,  z = sqrt(-2 ln u1) cos(2 pi u2) from Philox4x32-10 (key = seed, counter = x, y, projection, 0)
//
// The kernels.
//   conv3x3_mfma_kernel: an implicit GEMM on v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate: the reference's arithmetic,
//     only the order of summation differs), M = output pixels, N = C_out, K = 9 C_in.  The MFMA computes the transposed tile
//     (rows = output channels, columns = 32 pixels of one image row), so that a lane's accumulators are one pixel of 16 channels
//     and each store instruction writes 32 consecutive pixels.  A workgroup of 4 waves owns 8 rows x 32 columns of pixels and 32
//     or 64 output channels; a wave owns two of the rows.  K runs in chunks of 8 input channels: the 10 x 34 halo tile of the
//     chunk is staged in LDS with the coordinates clamped (= replicate padding), read from up to two channel-concatenated
//     sources, the second optionally through the x 2 nearest upsample (y >> 1, x >> 1) -- neither the concatenated nor the
//     upsampled tensor exists in memory.  The global loads of chunk k + 1 are issued into registers before the MFMAs of chunk k
//     and stored to LDS after them (staging them one load per wait cost 19 % of the network's convolution time).  The weights
//     are repacked once per call (pack_weights_kernel) into the order the kernel stages them in: per output-channel block and
//     chunk, [channel pair][tap][channel of the pair][output channel], padded with zeros to whole chunks and blocks, so that
//     one MFMA k-step takes the same tap of two neighbouring input channels and every LDS read has a compile-time offset.
//     Input channels past C_in are staged as zeros.  The bias is added in the epilogue.
//   Thin ends: NO layer takes a VALU kernel.  init_conv (C_in <= 2), the two final_conv (C_out = 1) and the 16/32-channel
//     variance net run on the same MFMA kernel with zero padding (C_out <= 32 takes the 32-channel variant).  Their padded
//     arithmetic is under 4 % of the mean net's; profiles/speedup_ab.md has the per-layer table.
//   stats_kernel + norm_lrelu_kernel: sum and sum of squares per channel in float64, over fixed segments and a fixed tree (no
//     atomics: the same input gives the same bytes), the normalisation applied in float64 and rounded once.  A pass of its own;
//     applying it when the next convolution stages its input was not tried.
//   maxpool_kernel, preprocess_kernel (statistics in float64 by stats_kernel, applied in float32), head_mean_kernel,
//     head_variance_kernel, sample_kernel.
// One projection at a time (the reference runs batch size 1 per sample in effect: instance norm keeps samples independent); the
// buffers of one projection are allocated once per call.  No graphs.
#include <chrono>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

using mcgpu::CallDevice;
using mcgpu::Stage;

[[noreturn]] void refuse(const char* fn, const std::string& what) { throw mcgpu::Error(-1, std::string("!!ERROR!! ") + fn + ": " + what); }

// ---------------------------------------------------------------------------------------------------------------- convolution
constexpr int kTileW = 32, kTileH = 8;                   // pixels of a workgroup: 4 waves x 2 rows x 32 columns
constexpr int kCK = 8;                                   // input channels per K chunk
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;  // the staged tile
constexpr int kHalo = kHaloW * kHaloH;
constexpr int kKK = kCK * 9;                             // K of a chunk

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
  const float* src1;   // [c1][H][W]
  const float* src2;   // [c2][H2][W2] or nullptr
  int c1, c2, H, W, H2, W2, ups;
  const float* wpack;  // [blocks of 32 NB output channels][n_chunks][kKK][32 NB]
  const float* bias;   // [c_out]
  float* out;          // [c_out][H][W]
  int c_out, n_chunks;
};

// w [c_out][c_in][3][3] -> the staging order of conv3x3_mfma_kernel<NB>, zero where the channel does not exist
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* w, float* wpack, int c_in, int c_out, int n_chunks, int ncol, size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int co_local = (int)(e % ncol);
  size_t r = e / ncol;
  const int kk = (int)(r % kKK);
  r /= kKK;
  const int ch = (int)(r % n_chunks), cb = (int)(r / n_chunks);
  const int hh = kk & 1, tap = (kk >> 1) % 9, cp = (kk >> 1) / 9;
  const int ci = ch * kCK + cp * 2 + hh, co = cb * ncol + co_local;
  wpack[e] = (ci < c_in && co < c_out) ? w[((size_t)co * c_in + ci) * 9 + tap] : 0.f;
}

// What one thread moves per K chunk, global -> registers -> LDS.  The loads of chunk k + 1 are issued before the MFMAs of chunk k and
// land during them; every load is unconditional (clamped index, value masked), so that they go out together and not one per wait.
constexpr int kStageIn = (kCK * kHalo + 255) / 256;

template <int NB> struct WeightWord;  // 32 NB kKK floats of weights per chunk = 9 words of NB floats for each of 256 threads, exactly
template <> struct WeightWord<1> { using T = float; };
template <> struct WeightWord<2> { using T = float2; };

template <int NB>
struct Staged {
  static constexpr int kW = kKK * 32 / 256;
  using Word = typename WeightWord<NB>::T;
  float in[kStageIn];
  Word w[kW];
};
static_assert(kKK * 32 % 256 == 0, "the weights of a chunk are whole words per thread");

template <int NB>
__device__ __forceinline__ void load_chunk(const ConvArgs& a, const float* wp, int ch, int tid, int x0, int y0, Staged<NB>& s) {
#pragma unroll
  for (int i = 0; i < kStageIn; ++i) {
    const int e = min(tid + i * 256, kCK * kHalo - 1);
    const int c = e / kHalo, r = e - c * kHalo, yy = r / kHaloW, xx = r - yy * kHaloW;
    const int gc = ch * kCK + c;
    const int y = min(max(y0 + yy - 1, 0), a.H - 1), x = min(max(x0 + xx - 1, 0), a.W - 1);  // replicate padding
    const bool first = gc < a.c1, any = gc < a.c1 + a.c2;
    const int cc = first ? gc : gc - a.c1, hh = first ? a.H : a.H2, ww = first ? a.W : a.W2, sh = first ? 0 : a.ups;
    const float* src = (first || !any) ? a.src1 : a.src2;
    const size_t idx = any ? ((size_t)cc * hh + (y >> sh)) * ww + (x >> sh) : 0;  // a channel past the last: any valid address, zeroed
    const float v = src[idx];
    s.in[i] = any ? v : 0.f;
  }
  const auto* wsrc = (const typename Staged<NB>::Word*)(wp + (size_t)ch * (kKK * 32 * NB));
#pragma unroll
  for (int i = 0; i < Staged<NB>::kW; ++i) s.w[i] = wsrc[tid + i * 256];
}

template <int NB>
__device__ __forceinline__ void store_chunk(const Staged<NB>& s, int tid, float* s_in, float* s_w) {
#pragma unroll
  for (int i = 0; i < kStageIn; ++i)
    if (tid + i * 256 < kCK * kHalo) s_in[tid + i * 256] = s.in[i];
#pragma unroll
  for (int i = 0; i < Staged<NB>::kW; ++i)
    ((typename Staged<NB>::Word*)s_w)[tid + i * 256] = s.w[i];
}

template <int NB>  // blocks of 32 output channels per workgroup
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(ConvArgs a) {
  __shared__ float s_in[kCK * kHalo];
  __shared__ __attribute__((aligned(16))) float s_w[kKK * 32 * NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, cb = blockIdx.z;
  f32x16 acc[2][NB];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rs][nb][r] = 0.f;
  const float* wp = a.wpack + (size_t)cb * a.n_chunks * (kKK * 32 * NB);
  const float* pin = s_in + h * kHalo + (2 * wave) * kHaloW + col;  // lane half h takes the odd channel of a pair
  const float* pw = s_w + h * (32 * NB) + col;
  Staged<NB> st;
  load_chunk<NB>(a, wp, 0, tid, x0, y0, st);
  for (int ch = 0; ch < a.n_chunks; ++ch) {
    store_chunk<NB>(st, tid, s_in, s_w);
    __syncthreads();
    if (ch + 1 < a.n_chunks) load_chunk<NB>(a, wp, ch + 1, tid, x0, y0, st);
#pragma unroll
    for (int cp = 0; cp < kCK / 2; ++cp)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap % 3;
        const float b0 = pin[cp * 2 * kHalo + dy * kHaloW + dx];
        const float b1 = pin[cp * 2 * kHalo + (dy + 1) * kHaloW + dx];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const float wv = pw[(cp * 9 + tap) * 2 * (32 * NB) + nb * 32];
          acc[0][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, b0, acc[0][nb], 0, 0, 0);
          acc[1][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, b1, acc[1][nb], 0, 0, 0);
        }
      }
    __syncthreads();
  }
  const int x = x0 + col;
  if (x >= a.W) return;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float bias[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias[r] = a.bias[min((cb * NB + nb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, a.c_out - 1)];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
      const int y = y0 + 2 * wave + rs;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = (cb * NB + nb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;  // the 32x32 C/D map: row of register r in lane half h
        if (y < a.H && co < a.c_out) a.out[((size_t)co * a.H + y) * a.W + x] = acc[rs][nb][r] + bias[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- instance norm + LeakyReLU
constexpr int kMaxSegments = 64;
constexpr size_t kSegmentPixels = 16384;

int segments_of(size_t hw) { return (int)std::min<size_t>(kMaxSegments, (hw + kSegmentPixels - 1) / kSegmentPixels); }

// part[c][s] = (sum, sum of squares) of segment s of channel c, in float64 and in a fixed order
__global__ __launch_bounds__(256) void stats_kernel(const float* x, size_t hw, int S, double2* part) {
  __shared__ double s_sum[256], s_sq[256];
  const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const size_t seg = (hw + S - 1) / S, lo = (size_t)s * seg, hi = min(lo + seg, hw);
  const float* p = x + (size_t)c * hw;
  double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};  // four chains: four loads in flight, the order still fixed
  size_t i = lo + tid;
  for (; i + 768 < hi; i += 1024) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = p[i + 256 * k];
      sum[k] += v;
      sq[k] += v * v;
    }
  }
  for (; i < hi; i += 256) {
    const double v = p[i];
    sum[0] += v;
    sq[0] += v * v;
  }
  s_sum[tid] = (sum[0] + sum[1]) + (sum[2] + sum[3]);
  s_sq[tid] = (sq[0] + sq[1]) + (sq[2] + sq[3]);
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_sum[tid] += s_sum[tid + w];
      s_sq[tid] += s_sq[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) part[(size_t)c * S + s] = make_double2(s_sum[0], s_sq[0]);
}

__device__ double2 fold_segments(const double2* part, int S) {
  double sum = 0.0, sq = 0.0;
  for (int s = 0; s < S; ++s) {
    sum += part[s].x;
    sq += part[s].y;
  }
  return make_double2(sum, sq);
}

__global__ __launch_bounds__(256) void norm_lrelu_kernel(const float* x, float* y, size_t hw, int S, const double2* part) {
  __shared__ double s_mean, s_rstd;
  const int c = blockIdx.y;
  if (threadIdx.x == 0) {
    const double2 t = fold_segments(part + (size_t)c * S, S);
    const double m = t.x / (double)hw, var = fmax(t.y / (double)hw - m * m, 0.0);
    s_mean = m;
    s_rstd = 1.0 / sqrt(var + 1e-5);
  }
  __syncthreads();
  const double m = s_mean, rstd = s_rstd;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const float v = (float)(((double)x[(size_t)c * hw + i] - m) * rstd);
  y[(size_t)c * hw + i] = v > 0.f ? v : 0.01f * v;
}

// ------------------------------------------------------------------------------------------------------------- small kernels
__global__ __launch_bounds__(256) void maxpool_kernel(const float* x, float* y, int C, int H, int W) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)C * Ho * Wo) return;
  const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho), c = (int)(i / ((size_t)Wo * Ho));
  const float* p = x + ((size_t)c * H + 2 * yo) * W + 2 * xo;
  y[i] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
}

// fp' = (fp - mean fp) / std fp * std lp + mean lp: statistics from float64 sums, applied in float32 as the reference does
__global__ __launch_bounds__(256) void preprocess_kernel(const float* fp, float* out, size_t hw, int S, const double2* part_lp, const double2* part_fp) {
  __shared__ float s_v[4];
  if (threadIdx.x < 2) {
    const double2 t = fold_segments(threadIdx.x ? part_fp : part_lp, S);
    const double m = t.x / (double)hw, var = fmax((t.y - t.x * m) / (double)(hw - 1), 0.0);
    s_v[2 * threadIdx.x] = (float)m;
    s_v[2 * threadIdx.x + 1] = (float)sqrt(var);
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  out[i] = (fp[i] - s_v[2]) / s_v[3] * s_v[1] + s_v[0];
}

__global__ __launch_bounds__(256) void head_mean_kernel(const float* low_photon, const float* net, float* mean, size_t hw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < hw) mean[i] = fmaxf(low_photon[i] + 10.f * tanhf(net[i]), 0.f);
}

__global__ __launch_bounds__(256) void head_variance_kernel(const float* mean, const float* net, float* variance, size_t hw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < hw) variance[i] = mean[i] * (0.10f * (1.f / (1.f + expf(-net[i])))) + 1e-6f;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): words 0 and 1 of the block
__device__ void philox10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& w0, unsigned& w1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w0 = c0;
  w1 = c1;
}

__device__ float standard_normal(int x, int y, unsigned projection, unsigned long long seed) {
  unsigned w0, w1;
  philox10((unsigned)x, (unsigned)y, projection, 0u, (unsigned)seed, (unsigned)(seed >> 32), w0, w1);
  const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(w1 >> 8) * 0x1p-24f;  // u1 in (0, 1], u2 in [0, 1)
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// sample = mean + sqrt(variance) z; with mean == nullptr: z alone
__global__ __launch_bounds__(256) void sample_kernel(const float* mean, const float* variance, float* out, int W, size_t hw, unsigned projection,
                                                     unsigned long long seed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const float z = standard_normal((int)(i % W), (int)(i / W), projection, seed);
  out[i] = mean ? mean[i] + sqrtf(variance[i]) * z : z;
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// -------------------------------------------------------------------------------------------------------------------- host
struct NetShape { int in_channels, levels, base; };

struct ConvLayer {
  int c_in = 0, c_out = 0;
  size_t w_off = 0, b_off = 0;  // in the flat weights
  int nb = 1, n_chunks = 0;
  float* wpack = nullptr;
  const float* bias = nullptr;
  size_t pack_floats() const { return (size_t)((c_out + 32 * nb - 1) / (32 * nb)) * n_chunks * kKK * 32 * nb; }
};

ConvLayer conv_layer(int c_in, int c_out, size_t& cursor) {
  ConvLayer l;
  l.c_in = c_in;
  l.c_out = c_out;
  l.w_off = cursor;
  cursor += (size_t)c_out * c_in * 9;
  l.b_off = cursor;
  cursor += (size_t)c_out;
  l.nb = c_out > 32 ? 2 : 1;
  l.n_chunks = (c_in + kCK - 1) / kCK;
  return l;
}

// the convolutions of one FlexUNet in the state dict's order: init, final, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0
struct NetLayers {
  NetShape s;
  ConvLayer init, final;
  std::vector<ConvLayer> enc, dec;  // [2 i], [2 i + 1] of level i
  NetLayers(const NetShape& shape, size_t& cursor) : s(shape), enc(2 * shape.levels), dec(2 * shape.levels) {
    const int F = s.base, L = s.levels;
    init = conv_layer(s.in_channels, F, cursor);
    final = conv_layer(F, 1, cursor);
    for (int i = 0; i < L; ++i) {
      const int out = F << i, in = i ? F << (i - 1) : F;
      enc[2 * i] = conv_layer(in, out, cursor);
      enc[2 * i + 1] = conv_layer(out, out, cursor);
    }
    for (int i = L - 1; i >= 0; --i) {
      const int out = F << i, skip = i ? F << (i - 1) : F, below = i == L - 1 ? F << (L - 1) : F << (i + 1);
      dec[2 * i] = conv_layer(skip + below, out, cursor);
      dec[2 * i + 1] = conv_layer(out, out, cursor);
    }
  }
  template <class F>
  void each(F f) {
    f(init);
    f(final);
    for (auto& l : enc) f(l);
    for (auto& l : dec) f(l);
  }
};

struct Runner {
  CallDevice dev;
  mcgpu_speedup_report rep;
  double2* d_part = nullptr;   // statistics of the widest layer
  double2* d_part2 = nullptr;  // the second image of the preprocessing
  int max_channels = 1;

  Runner() { memset(&rep, 0, sizeof rep); }
  void init(int device, int channels) {
    HIP_TRY(hipSetDevice(device));
    dev.events();
    max_channels = std::max(channels, 1);
    d_part = dev.alloc_zeroed<double2>((size_t)max_channels * kMaxSegments * sizeof(double2));
    d_part2 = dev.alloc_zeroed<double2>(kMaxSegments * sizeof(double2));
  }
  float* alloc(size_t floats) { return dev.alloc_zeroed<float>(std::max<size_t>(floats, 1) * sizeof(float)); }

  void pack(ConvLayer& l, const float* d_weights) {
    const size_t total = l.pack_floats();
    l.wpack = dev.alloc<float>(total * sizeof(float));
    l.bias = d_weights + l.b_off;
    hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks_of(total)), dim3(256), 0, nullptr, d_weights + l.w_off, l.wpack, l.c_in, l.c_out, l.n_chunks,
                       32 * l.nb, total);
  }

  // out [c_out][H][W] = conv(cat(src1 [c1], src2 [c_in - c1] (upsampled when ups))) + bias
  void conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, int H, int W, float* out) {
    Stage st(dev, rep.ms_conv);
    ConvArgs a;
    a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = l.c_in - c1; a.H = H; a.W = W; a.ups = ups ? 1 : 0;
    a.H2 = ups ? (H + 1) / 2 : H; a.W2 = ups ? (W + 1) / 2 : W;
    a.wpack = l.wpack; a.bias = l.bias; a.out = out; a.c_out = l.c_out; a.n_chunks = l.n_chunks;
    const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)((l.c_out + 32 * l.nb - 1) / (32 * l.nb)));
    if (l.nb == 2) hipLaunchKernelGGL(conv3x3_mfma_kernel<2>, grid, dim3(256), 0, nullptr, a);
    else hipLaunchKernelGGL(conv3x3_mfma_kernel<1>, grid, dim3(256), 0, nullptr, a);
    st.done();
  }
  void stats(const float* x, int C, size_t hw, double2* part) {
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)segments_of(hw), (unsigned)C), dim3(256), 0, nullptr, x, hw, segments_of(hw), part);
  }
  void norm_lrelu(const float* x, float* y, int C, size_t hw) {
    Stage st(dev, rep.ms_norm);
    stats(x, C, hw, d_part);
    hipLaunchKernelGGL(norm_lrelu_kernel, dim3(blocks_of(hw), (unsigned)C), dim3(256), 0, nullptr, x, y, hw, segments_of(hw), d_part);
    st.done();
  }
  void maxpool(const float* x, float* y, int C, int H, int W) {
    Stage st(dev, rep.ms_other);
    const size_t n = (size_t)C * (H / 2) * (W / 2);
    if (n) hipLaunchKernelGGL(maxpool_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, y, C, H, W);
    st.done();
  }
  void preprocess(const float* lp, const float* fp, float* out, size_t hw) {
    Stage st(dev, rep.ms_preprocess);
    stats(lp, 1, hw, d_part);
    stats(fp, 1, hw, d_part2);
    hipLaunchKernelGGL(preprocess_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, fp, out, hw, segments_of(hw), d_part, d_part2);
    st.done();
  }
  void normals(const float* mean, const float* variance, float* out, int W, size_t hw, unsigned projection, unsigned long long seed) {
    Stage st(dev, rep.ms_other);
    hipLaunchKernelGGL(sample_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, mean, variance, out, W, hw, projection, seed);
    st.done();
  }
};

// One FlexUNet at one image size: its buffers, made once, and the launches of a forward pass
struct NetPass {
  NetLayers& net;
  Runner& run;
  int H, W;
  std::vector<float*> skip, pooled, enc_a, dec_a, dec_b;
  float* out = nullptr;
  NetPass(NetLayers& n, Runner& r, int h, int w) : net(n), run(r), H(h), W(w) {
    const int L = net.s.levels, F = net.s.base;
    skip.resize(L + 1); pooled.resize(L); enc_a.resize(L); dec_a.resize(L); dec_b.resize(L);
    skip[0] = run.alloc((size_t)F * H * W);
    for (int i = 0; i < L; ++i) {
      const size_t px = (size_t)(H >> (i + 1)) * (W >> (i + 1));
      pooled[i] = run.alloc((size_t)(i ? F << (i - 1) : F) * px);
      enc_a[i] = run.alloc((size_t)(F << i) * px);
      skip[i + 1] = run.alloc((size_t)(F << i) * px);
      dec_a[i] = run.alloc((size_t)(F << i) * (H >> i) * (W >> i));
      dec_b[i] = run.alloc((size_t)(F << i) * (H >> i) * (W >> i));
    }
    out = run.alloc((size_t)H * W);
  }
  const float* forward(const float* x) {
    const int L = net.s.levels, F = net.s.base;
    run.conv(net.init, x, net.s.in_channels, nullptr, 0, H, W, skip[0]);
    for (int i = 0; i < L; ++i) {
      const int h = H >> (i + 1), w = W >> (i + 1), c_in = i ? F << (i - 1) : F, c = F << i;
      run.maxpool(skip[i], pooled[i], c_in, H >> i, W >> i);
      run.conv(net.enc[2 * i], pooled[i], c_in, nullptr, 0, h, w, enc_a[i]);
      run.norm_lrelu(enc_a[i], enc_a[i], c, (size_t)h * w);
      run.conv(net.enc[2 * i + 1], enc_a[i], c, nullptr, 0, h, w, skip[i + 1]);
      run.norm_lrelu(skip[i + 1], skip[i + 1], c, (size_t)h * w);
    }
    const float* cur = skip[L];
    for (int i = L - 1; i >= 0; --i) {
      const int h = H >> i, w = W >> i, c_skip = i ? F << (i - 1) : F, c = F << i;
      run.conv(net.dec[2 * i], skip[i], c_skip, cur, 1, h, w, dec_a[i]);
      run.norm_lrelu(dec_a[i], dec_a[i], c, (size_t)h * w);
      run.conv(net.dec[2 * i + 1], dec_a[i], c, nullptr, 0, h, w, dec_b[i]);
      run.norm_lrelu(dec_b[i], dec_b[i], c, (size_t)h * w);
      cur = dec_b[i];
    }
    run.conv(net.final, cur, F, nullptr, 0, H, W, out);
    return out;
  }
};

void read_options(const char* fn, const mcgpu_speedup_options* caller, mcgpu_speedup_options& o) {
  mcgpu::read_options(fn, "mcgpu_speedup_options", caller, o);
  if (o.n < 1 || o.nu < 1 || o.nv < 1) refuse(fn, "n, nu and nv must be >= 1");
  if ((unsigned long long)o.nu * (unsigned long long)o.nv > 0x7fffffffull) refuse(fn, "nu x nv must be below 2^31");
}

bool shape_ok(const NetShape& s) { return s.levels >= 1 && s.levels <= 8 && s.base >= 1 && s.base <= 1024 && s.in_channels >= 1; }

void check_run(const mcgpu_speedup_options& o, const float* low_photon, const float* forward_projection) {
  const char* fn = "mcgpu_speedup_run";
  if (!low_photon) refuse(fn, "low_photon is NULL");
  if (!o.weights) refuse(fn, "weights is NULL");
  const NetShape m{o.mean_in_channels, o.mean_levels, o.mean_filter_base}, v{o.var_in_channels, o.var_levels, o.var_filter_base};
  if (!shape_ok(m) || !shape_ok(v) || m.in_channels > 2 || v.in_channels != 1)
    refuse(fn, "bad architecture: mean_in_channels 1 or 2, var_in_channels 1, levels 1..8, filter_base 1..1024");
  if (m.in_channels == 2 && !forward_projection) refuse(fn, "forward_projection is NULL but the mean net has 2 input channels");
  if (m.in_channels == 1 && forward_projection) refuse(fn, "the mean net has 1 input channel: forward_projection must be NULL");
  size_t expect = 0;
  NetLayers(m, expect);
  NetLayers(v, expect);
  if (o.n_weights != expect)
    refuse(fn, "n_weights is " + std::to_string(o.n_weights) + " but the architecture has " + std::to_string(expect) + " values");
  const int deep = std::max(m.levels, v.levels);
  if (o.nu % (1 << deep) || o.nv % (1 << deep))
    refuse(fn, "nu and nv must be divisible by " + std::to_string(1 << deep) + " (2^levels): " + std::to_string(o.nu) + " x " + std::to_string(o.nv));
  if ((size_t)(o.nu >> deep) * (o.nv >> deep) < 2)
    refuse(fn, "the bottleneck of a " + std::to_string(o.nu) + " x " + std::to_string(o.nv) + " image has fewer than 2 pixels: instance norm is undefined");
  if (forward_projection) {
    const size_t hw = (size_t)o.nu * o.nv;
    for (int p = 0; p < o.n; ++p) {
      const float* s = forward_projection + (size_t)p * hw;
      size_t i = 1;
      while (i < hw && s[i] == s[0]) ++i;
      if (i == hw) refuse(fn, "forward_projection slice " + std::to_string(p) + " has zero variance: it cannot be matched to the low-photon projection");
    }
  }
}

void finish(Runner& R, const std::chrono::steady_clock::time_point& t0, mcgpu_speedup_report* report) {
  R.rep.peak_device_bytes = R.dev.peak;
  R.rep.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (report) *report = R.rep;
}

}  // namespace

extern "C" int mcgpu_speedup_run(const mcgpu_speedup_options* caller_o, const float* low_photon, const float* forward_projection, float* mean,
                                 float* variance, float* sample, mcgpu_speedup_report* report) {
  ABI_BEGIN
  mcgpu_speedup_options o;
  read_options("mcgpu_speedup_run", caller_o, o);
  check_run(o, low_photon, forward_projection);
  const auto t0 = std::chrono::steady_clock::now();
  size_t cursor = 0;
  NetLayers mean_net({o.mean_in_channels, o.mean_levels, o.mean_filter_base}, cursor);
  NetLayers var_net({o.var_in_channels, o.var_levels, o.var_filter_base}, cursor);
  Runner R;
  R.init(o.device, std::max(o.mean_filter_base << (o.mean_levels - 1), o.var_filter_base << (o.var_levels - 1)));
  const int H = o.nv, W = o.nu;
  const size_t hw = (size_t)H * W;
  float *d_x, *d_fp, *d_mean, *d_var, *d_sample;
  {
    Stage st(R.dev, R.rep.ms_upload);
    const float* d_weights = R.dev.upload(o.weights, (size_t)o.n_weights);
    mean_net.each([&](ConvLayer& l) { R.pack(l, d_weights); });
    var_net.each([&](ConvLayer& l) { R.pack(l, d_weights); });
    st.done();
  }
  d_x = R.alloc(2 * hw);  // channel 0: the low-photon projection, channel 1: the matched forward projection
  d_fp = R.alloc(hw);
  d_mean = R.alloc(hw);
  d_var = R.alloc(hw);
  d_sample = R.alloc(hw);
  NetPass mean_pass(mean_net, R, H, W), var_pass(var_net, R, H, W);
  for (int p = 0; p < o.n; ++p) {
    {
      Stage st(R.dev, R.rep.ms_upload);
      HIP_TRY(hipMemcpy(d_x, low_photon + (size_t)p * hw, hw * 4, hipMemcpyHostToDevice));
      if (forward_projection) HIP_TRY(hipMemcpy(d_fp, forward_projection + (size_t)p * hw, hw * 4, hipMemcpyHostToDevice));
      st.done();
    }
    if (forward_projection) R.preprocess(d_x, d_fp, d_x + hw, hw);
    const float* net_mean = mean_pass.forward(d_x);
    {
      Stage st(R.dev, R.rep.ms_other);
      hipLaunchKernelGGL(head_mean_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_x, net_mean, d_mean, hw);
      st.done();
    }
    const float* net_var = var_pass.forward(d_mean);
    {
      Stage st(R.dev, R.rep.ms_other);
      hipLaunchKernelGGL(head_variance_kernel, dim3(blocks_of(hw)), dim3(256), 0, nullptr, d_mean, net_var, d_var, hw);
      st.done();
    }
    if (sample) R.normals(d_mean, d_var, d_sample, W, hw, (unsigned)(o.first_projection + p), o.seed);
    {
      Stage st(R.dev, R.rep.ms_upload);
      if (mean) HIP_TRY(hipMemcpy(mean + (size_t)p * hw, d_mean, hw * 4, hipMemcpyDeviceToHost));
      if (variance) HIP_TRY(hipMemcpy(variance + (size_t)p * hw, d_var, hw * 4, hipMemcpyDeviceToHost));
      if (sample) HIP_TRY(hipMemcpy(sample + (size_t)p * hw, d_sample, hw * 4, hipMemcpyDeviceToHost));
      st.done();
    }
  }
  finish(R, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_speedup_stage(const mcgpu_speedup_options* caller_o, int stage, const mcgpu_speedup_stage_args* caller_a, mcgpu_speedup_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_speedup_stage";
  mcgpu_speedup_options o;
  read_options(fn, caller_o, o);
  mcgpu_speedup_stage_args a;
  mcgpu::read_options(fn, "mcgpu_speedup_stage_args", caller_a, a);
  if (stage < MCGPU_SPEEDUP_STAGE_CONV || stage > MCGPU_SPEEDUP_STAGE_NORMALS) refuse(fn, "unknown stage " + std::to_string(stage));
  if (!a.out) refuse(fn, "out is NULL");
  if (stage != MCGPU_SPEEDUP_STAGE_NORMALS && !a.in) refuse(fn, "in is NULL");
  const int H = o.nv, W = o.nu;
  const size_t hw = (size_t)H * W;
  if (stage <= MCGPU_SPEEDUP_STAGE_MAXPOOL && (a.c1 < 1 || a.c1 > 65536)) refuse(fn, "c1 must be 1..65536");
  if (stage == MCGPU_SPEEDUP_STAGE_CONV) {
    if (a.c2 < 0 || a.c2 > 65536 || a.c_out < 1 || a.c_out > 65536) refuse(fn, "c2 must be 0..65536 and c_out 1..65536");
    if (!a.weight || !a.bias) refuse(fn, "weight or bias is NULL");
    if (a.c2 > 0 && !a.in2) refuse(fn, "in2 is NULL");
  }
  if (stage == MCGPU_SPEEDUP_STAGE_NORM_LRELU && hw < 2) refuse(fn, "instance norm needs at least 2 pixels");
  if (stage == MCGPU_SPEEDUP_STAGE_PREPROCESS && (!a.in2 || hw < 2)) refuse(fn, "in2 is NULL or the image has fewer than 2 pixels");
  const auto t0 = std::chrono::steady_clock::now();
  Runner R;
  R.init(o.device, stage == MCGPU_SPEEDUP_STAGE_NORM_LRELU ? a.c1 : 1);
  switch (stage) {
    case MCGPU_SPEEDUP_STAGE_CONV: {
      const int H2 = a.upsample ? (H + 1) / 2 : H, W2 = a.upsample ? (W + 1) / 2 : W;
      size_t cursor = 0;
      ConvLayer l = conv_layer(a.c1 + a.c2, a.c_out, cursor);
      std::vector<float> flat(cursor);
      memcpy(flat.data() + l.w_off, a.weight, (size_t)l.c_out * l.c_in * 9 * sizeof(float));
      memcpy(flat.data() + l.b_off, a.bias, (size_t)l.c_out * sizeof(float));
      const float* d_weights = R.dev.upload(flat);
      R.pack(l, d_weights);
      const float* d_in = R.dev.upload(a.in, (size_t)a.c1 * hw);
      const float* d_in2 = a.c2 ? R.dev.upload(a.in2, (size_t)a.c2 * H2 * W2) : nullptr;
      float* d_out = R.alloc((size_t)a.c_out * hw);
      R.conv(l, d_in, a.c1, d_in2, a.upsample, H, W, d_out);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)a.c_out * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SPEEDUP_STAGE_NORM_LRELU: {
      const float* d_in = R.dev.upload(a.in, (size_t)a.c1 * hw);
      float* d_out = R.alloc((size_t)a.c1 * hw);
      R.norm_lrelu(d_in, d_out, a.c1, hw);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)a.c1 * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SPEEDUP_STAGE_MAXPOOL: {
      const size_t n_out = (size_t)a.c1 * (H / 2) * (W / 2);
      const float* d_in = R.dev.upload(a.in, (size_t)a.c1 * hw);
      float* d_out = R.alloc(n_out);
      R.maxpool(d_in, d_out, a.c1, H, W);
      if (n_out) HIP_TRY(hipMemcpy(a.out, d_out, n_out * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SPEEDUP_STAGE_PREPROCESS: {
      const float* d_lp = R.dev.upload(a.in, (size_t)o.n * hw);
      const float* d_fp = R.dev.upload(a.in2, (size_t)o.n * hw);
      float* d_out = R.alloc((size_t)o.n * hw);
      for (int p = 0; p < o.n; ++p) R.preprocess(d_lp + (size_t)p * hw, d_fp + (size_t)p * hw, d_out + (size_t)p * hw, hw);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)o.n * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    default: {
      float* d_out = R.alloc((size_t)o.n * hw);
      for (int p = 0; p < o.n; ++p) R.normals(nullptr, nullptr, d_out + (size_t)p * hw, W, hw, (unsigned)(o.first_projection + p), o.seed);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)o.n * hw * 4, hipMemcpyDeviceToHost));
    }
  }
  finish(R, t0, report);
  return 0;
  ABI_END
}
