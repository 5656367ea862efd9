// speedup_conv.inc -- what speedup_net.hip (inference) and speedup_train.hip (training) share of the 2-D speed-up network: the MFMA
// convolution, the max-pool, the preprocessing and the two heads, the shape of a FlexUNet as unet_common.inc's NetLayers, and the
// launches of those kernels.  Included inside each file's unnamed namespace, after unet_common.inc (kTaps = 9).  speedup_net.hip's
// header describes the kernels.
//
// conv3x3_mfma_kernel<NB, ZERO>.  ZERO = false is the forward convolution: coordinates clamped (replicate padding), up to two
// channel-concatenated sources.  ZERO = true is the same implicit GEMM for the input gradient (speedup_train.hip): one source of
// H2 x W2 pixels staged with zeros outside it, evaluated on the (H2 + 2) x (W2 + 2) pixels that the clamp reads from: output pixel
// (y, x) is the correlation centred on source pixel (y - 1, x - 1).  Only the forward instantiations exist in speedup_net.hip.

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

template <int NB, bool ZERO>
__device__ __forceinline__ void load_chunk(const ConvArgs& a, const float* wp, int ch, int tid, int x0, int y0, Staged<NB>& s) {
#pragma unroll
  for (int i = 0; i < kStageIn; ++i) {
    const int e = min(tid + i * 256, kCK * kHalo - 1);
    const int c = e / kHalo, r = e - c * kHalo, yy = r / kHaloW, xx = r - yy * kHaloW;
    const int gc = ch * kCK + c;
    if constexpr (ZERO) {
      const int y = y0 + yy - 2, x = x0 + xx - 2;  // zero padding, one pixel further out
      const bool any = gc < a.c1 && y >= 0 && y < a.H2 && x >= 0 && x < a.W2;
      const size_t idx = any ? ((size_t)gc * a.H2 + y) * a.W2 + x : 0;
      const float v = a.src1[idx];
      s.in[i] = any ? v : 0.f;
    } else {
      const int y = min(max(y0 + yy - 1, 0), a.H - 1), x = min(max(x0 + xx - 1, 0), a.W - 1);  // replicate padding
      const bool first = gc < a.c1, any = gc < a.c1 + a.c2;
      const int cc = first ? gc : gc - a.c1, hh = first ? a.H : a.H2, ww = first ? a.W : a.W2, sh = first ? 0 : a.ups;
      const float* src = (first || !any) ? a.src1 : a.src2;
      const size_t idx = any ? ((size_t)cc * hh + (y >> sh)) * ww + (x >> sh) : 0;  // a channel past the last: any valid address, zeroed
      const float v = src[idx];
      s.in[i] = any ? v : 0.f;
    }
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

template <int NB, bool ZERO = false>  // NB: blocks of 32 output channels per workgroup
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
  load_chunk<NB, ZERO>(a, wp, 0, tid, x0, y0, st);
  for (int ch = 0; ch < a.n_chunks; ++ch) {
    store_chunk<NB>(st, tid, s_in, s_w);
    __syncthreads();
    if (ch + 1 < a.n_chunks) load_chunk<NB, ZERO>(a, wp, ch + 1, tid, x0, y0, st);
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

bool shape_ok(const NetShape& s) { return s.levels >= 1 && s.levels <= 8 && s.base >= 1 && s.base <= 1024 && s.in_channels >= 1; }

// the first forward-projection slice of zero variance, or -1: such a slice cannot be matched to the low-photon projection
int constant_slice(const float* forward_projection, int n, size_t hw) {
  for (int p = 0; p < n; ++p) {
    const float* s = forward_projection + (size_t)p * hw;
    size_t i = 1;
    while (i < hw && s[i] == s[0]) ++i;
    if (i == hw) return p;
  }
  return -1;
}

// out [c_out][H][W] = conv(cat(src1 [c1], src2 [c_in - c1] (upsampled when ups))) + bias
void launch_conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, const Dims& D, float* out) {
  const Dims E = ups ? D.halved_up() : D;
  ConvArgs a;
  a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = l.c_in - c1; a.H = D.H; a.W = D.W; a.ups = ups ? 1 : 0;
  a.H2 = E.H; a.W2 = E.W;
  a.wpack = l.wpack; a.bias = l.bias; a.out = out; a.c_out = l.c_out; a.n_chunks = l.n_chunks;
  const dim3 grid((unsigned)((D.W + kTileW - 1) / kTileW), (unsigned)((D.H + kTileH - 1) / kTileH), (unsigned)((l.c_out + 32 * l.nb - 1) / (32 * l.nb)));
  if (l.nb == 2) hipLaunchKernelGGL((conv3x3_mfma_kernel<2>), grid, dim3(256), 0, nullptr, a);
  else hipLaunchKernelGGL((conv3x3_mfma_kernel<1>), grid, dim3(256), 0, nullptr, a);
}

void launch_maxpool(const float* x, float* y, int C, const Dims& D) {
  const size_t n = (size_t)C * D.shifted(1).voxels();
  if (n) hipLaunchKernelGGL(maxpool_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, y, C, D.H, D.W);
}
