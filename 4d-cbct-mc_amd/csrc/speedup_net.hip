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
//   Instance norm (stats_kernel + norm_lrelu_kernel: float64 sums over fixed segments and a fixed tree, normalised in float64, rounded
//     once), the packing of the weights, the plan of the layers and the launches of a forward pass are unet_common.inc's, shared with
//     segment_net.hip.  The norm is a pass of its own; applying it when the next convolution stages its input was not tried.
//   maxpool_kernel, preprocess_kernel (statistics in float64 by stats_kernel, applied in float32), head_mean_kernel,
//     head_variance_kernel, sample_kernel.
// One projection at a time (the reference runs batch size 1 per sample in effect: instance norm keeps samples independent); the
// buffers of one projection are allocated once per call.  No graphs.
#include <chrono>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

constexpr int kTaps = 9;  // 3 x 3: what unet_common.inc sizes a K chunk and counts the weights with
#include "unet_common.inc"

// ---------------------------------------------------------------------------------------------------------------- convolution
constexpr int kTileW = 32, kTileH = 8;                   // pixels of a workgroup: 4 waves x 2 rows x 32 columns
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;  // the staged tile
constexpr int kHalo = kHaloW * kHaloH;

struct ConvArgs {
  const float* src1;   // [c1][H][W]
  const float* src2;   // [c2][H2][W2] or nullptr
  int c1, c2, H, W, H2, W2, ups;
  const float* wpack;  // [blocks of 32 NB output channels][n_chunks][kKK][32 NB]
  const float* bias;   // [c_out]
  float* out;          // [c_out][H][W]
  int c_out, n_chunks;
};

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

// -------------------------------------------------------------------------------------------------------------------- host
struct Dims {
  int H, W;
  size_t voxels() const { return (size_t)H * W; }
  Dims shifted(int s) const { return {H >> s, W >> s}; }
  Dims halved_up() const { return {(H + 1) / 2, (W + 1) / 2}; }
};

struct NetShape { int in_channels, levels, base; };

// FlexUNet(C, L, base F) as unet_common.inc's NetLayers: init F, enc_i and dec_i F 2^i, final F, one class
NetLayers layers_of(const NetShape& s, size_t& cursor) {
  std::vector<int> f{s.base};
  for (int i = 0; i < s.levels; ++i) f.push_back(s.base << i);
  for (int i = s.levels - 1; i >= 0; --i) f.push_back(s.base << i);
  f.push_back(s.base);
  return NetLayers(s.in_channels, s.levels, f.data(), 1, cursor);
}

int blocks_per_workgroup(int c_out) { return c_out > 32 ? 2 : 1; }  // of 32 output channels: the variant of conv3x3_mfma_kernel

struct Runner : RunnerBase<mcgpu_speedup_report> {
  double2* d_part2 = nullptr;  // the second image of the preprocessing

  void init(int device, int channels) {
    RunnerBase::init(device, channels);
    d_part2 = (double2*)alloc_bytes(kMaxSegments * sizeof(double2), true);
  }
  void pack_net(NetLayers& net, const float* d_weights) {
    net.each([&](ConvLayer& l) {
      l.nb = blocks_per_workgroup(l.c_out);
      pack(l, d_weights);
    });
  }

  // out [c_out][H][W] = conv(cat(src1 [c1], src2 [c_in - c1] (upsampled when ups))) + bias
  void conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, const Dims& D, float* out) {
    Stage st(dev, rep.ms_conv);
    const Dims E = ups ? D.halved_up() : D;
    ConvArgs a;
    a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = l.c_in - c1; a.H = D.H; a.W = D.W; a.ups = ups ? 1 : 0;
    a.H2 = E.H; a.W2 = E.W;
    a.wpack = l.wpack; a.bias = l.bias; a.out = out; a.c_out = l.c_out; a.n_chunks = l.n_chunks;
    const dim3 grid((unsigned)((D.W + kTileW - 1) / kTileW), (unsigned)((D.H + kTileH - 1) / kTileH), (unsigned)((l.c_out + 32 * l.nb - 1) / (32 * l.nb)));
    if (l.nb == 2) hipLaunchKernelGGL(conv3x3_mfma_kernel<2>, grid, dim3(256), 0, nullptr, a);
    else hipLaunchKernelGGL(conv3x3_mfma_kernel<1>, grid, dim3(256), 0, nullptr, a);
    st.done();
  }
  void maxpool(const float* x, float* y, int C, const Dims& D) {
    Stage st(dev, rep.ms_other);
    const size_t n = (size_t)C * D.shifted(1).voxels();
    if (n) hipLaunchKernelGGL(maxpool_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, y, C, D.H, D.W);
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
  layers_of(m, expect);
  layers_of(v, expect);
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

}  // namespace

extern "C" int mcgpu_speedup_run(const mcgpu_speedup_options* caller_o, const float* low_photon, const float* forward_projection, float* mean,
                                 float* variance, float* sample, mcgpu_speedup_report* report) {
  ABI_BEGIN
  mcgpu_speedup_options o;
  read_options("mcgpu_speedup_run", caller_o, o);
  check_run(o, low_photon, forward_projection);
  const auto t0 = std::chrono::steady_clock::now();
  size_t cursor = 0;
  NetLayers mean_net = layers_of({o.mean_in_channels, o.mean_levels, o.mean_filter_base}, cursor);
  NetLayers var_net = layers_of({o.var_in_channels, o.var_levels, o.var_filter_base}, cursor);
  Runner R;
  R.init(o.device, std::max(mean_net.widest(), var_net.widest()));
  const Dims D{o.nv, o.nu};
  const size_t hw = D.voxels();
  float *d_x, *d_fp, *d_mean, *d_var, *d_sample;
  {
    Stage st(R.dev, R.rep.ms_upload);
    const float* d_weights = R.upload(o.weights, (size_t)o.n_weights);
    R.pack_net(mean_net, d_weights);
    R.pack_net(var_net, d_weights);
    st.done();
  }
  d_x = R.alloc(2 * hw);  // channel 0: the low-photon projection, channel 1: the matched forward projection
  d_fp = R.alloc(hw);
  d_mean = R.alloc(hw);
  d_var = R.alloc(hw);
  d_sample = R.alloc(hw);
  NetPass<Runner, Dims> mean_pass(mean_net, R, D), var_pass(var_net, R, D);
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
    if (sample) R.normals(d_mean, d_var, d_sample, D.W, hw, (unsigned)(o.first_projection + p), o.seed);
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
  const Dims D{o.nv, o.nu};
  const size_t hw = D.voxels();
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
    case MCGPU_SPEEDUP_STAGE_CONV: stage_conv(R, a, D, blocks_per_workgroup(a.c_out)); break;
    case MCGPU_SPEEDUP_STAGE_NORM_LRELU: stage_norm_lrelu(R, a, hw); break;
    case MCGPU_SPEEDUP_STAGE_MAXPOOL: stage_maxpool(R, a, D); break;
    case MCGPU_SPEEDUP_STAGE_PREPROCESS: {
      const float* d_lp = R.upload(a.in, (size_t)o.n * hw);
      const float* d_fp = R.upload(a.in2, (size_t)o.n * hw);
      float* d_out = R.alloc((size_t)o.n * hw);
      for (int p = 0; p < o.n; ++p) R.preprocess(d_lp + (size_t)p * hw, d_fp + (size_t)p * hw, d_out + (size_t)p * hw, hw);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)o.n * hw * 4, hipMemcpyDeviceToHost));
      break;
    }
    default: {
      float* d_out = R.alloc((size_t)o.n * hw);
      for (int p = 0; p < o.n; ++p) R.normals(nullptr, nullptr, d_out + (size_t)p * hw, D.W, hw, (unsigned)(o.first_projection + p), o.seed);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)o.n * hw * 4, hipMemcpyDeviceToHost));
    }
  }
  finish(R, t0, report);
  return 0;
  ABI_END
}
