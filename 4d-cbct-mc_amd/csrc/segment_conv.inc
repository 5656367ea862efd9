// segment_conv.inc -- the forward kernels of the 3-D segmentation network that segment_net.hip (inference) and segment_train.hip
// (training: the forward pass, and the input gradient as the same convolution with a second packing of the weights) share:
// conv3x3x3_mfma_kernel with its staging, maxpool3d_kernel, head_kernel, the extent type Dims and the two launches.  segment_net.hip's
// header describes the convolution.  Included inside each file's unnamed namespace, after unet_common.inc with kTaps = 27.

struct Dims {
  int d[3];
  size_t voxels() const { return (size_t)d[0] * d[1] * d[2]; }
  Dims shifted(int s) const { return {{d[0] >> s, d[1] >> s, d[2] >> s}}; }
  Dims halved_up() const { return {{(d[0] + 1) / 2, (d[1] + 1) / 2, (d[2] + 1) / 2}}; }
};

// ---------------------------------------------------------------------------------------------------------------- convolution
constexpr int kT0 = 2, kT1 = 4, kT2 = 32;                        // voxels of a workgroup: 4 waves x 2 d1-rows x 32
constexpr int kH0 = kT0 + 2, kH1 = kT1 + 2, kH2 = kT2 + 2;       // the staged tile
constexpr int kHalo = kH0 * kH1 * kH2;

struct ConvArgs {
  const float* src1;   // [c1][D0][D1][D2]
  const float* src2;   // [c2][E0][E1][E2] or nullptr
  int c1, c2, D0, D1, D2, E0, E1, E2, ups;
  const float* wpack;  // [blocks of 32 output channels][n_chunks][kKK][32]
  const float* bias;   // [c_out]
  float* out;          // [c_out][D0][D1][D2]
  int c_out, n_chunks, nb2;  // nb2: workgroups along d2; blockIdx.x = block along d2 + nb2 * block of output channels
};

constexpr int kSlots = (kHalo + 255) / 256;                      // halo positions of one channel a thread moves
constexpr int kStageW = kKK * 32 / 256;                          // floats of the weights a thread moves per chunk
static_assert(kKK * 32 % 256 == 0, "the weights of a chunk are whole words per thread");

struct Staged {
  float in[kCK * kSlots];
  float w[kStageW];
};

// Where a thread's halo positions lie in a channel of either source (32-bit: a channel has fewer than 2^31 voxels, the host checks),
// worked out once: the chunks differ only in the channel, which is uniform over the workgroup.
struct HaloMap {
  unsigned off1[kSlots], off2[kSlots];
  unsigned ok;  // bit j: a position of the halo that lies inside the tensor: the others are the zero padding
};

__device__ __forceinline__ void map_halo(const ConvArgs& a, int tid, int x0, int y0, int z0, HaloMap& m) {
  m.ok = 0;
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int r = min(tid + j * 256, kHalo - 1);
    const int zz = r / (kH1 * kH2), r2 = r - zz * (kH1 * kH2), yy = r2 / kH2, xx = r2 - yy * kH2;
    const int z = z0 + zz - 1, y = y0 + yy - 1, x = x0 + xx - 1;
    if (tid + j * 256 < kHalo && z >= 0 && z < a.D0 && y >= 0 && y < a.D1 && x >= 0 && x < a.D2) m.ok |= 1u << j;
    const int zc = min(max(z, 0), a.D0 - 1), yc = min(max(y, 0), a.D1 - 1), xc = min(max(x, 0), a.D2 - 1);
    m.off1[j] = ((unsigned)zc * a.D1 + yc) * a.D2 + xc;
    m.off2[j] = ((unsigned)(zc >> a.ups) * a.E1 + (yc >> a.ups)) * a.E2 + (xc >> a.ups);
  }
}

// Every load is unconditional (clamped index, value masked), so that the loads of a chunk go out together.
__device__ __forceinline__ void load_chunk(const ConvArgs& a, const float* wp, int ch, int tid, const HaloMap& m, Staged& s) {
  const size_t n1 = ((size_t)a.D0 * a.D1) * a.D2, n2 = ((size_t)a.E0 * a.E1) * a.E2;
#pragma unroll
  for (int c = 0; c < kCK; ++c) {
    const int gc = ch * kCK + c;
    const bool first = gc < a.c1, any = gc < a.c1 + a.c2;
    const float* base = first ? a.src1 + (size_t)gc * n1 : any ? a.src2 + (size_t)(gc - a.c1) * n2 : a.src1;  // past the last: any valid address
    if (first || !any) {  // uniform over the workgroup
#pragma unroll
      for (int j = 0; j < kSlots; ++j) s.in[c * kSlots + j] = base[m.off1[j]];
    } else {
#pragma unroll
      for (int j = 0; j < kSlots; ++j) s.in[c * kSlots + j] = base[m.off2[j]];
    }
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
      if (!(any && (m.ok >> j & 1u))) s.in[c * kSlots + j] = 0.f;
  }
  const float* wsrc = wp + (size_t)ch * (kKK * 32);
#pragma unroll
  for (int i = 0; i < kStageW; ++i) s.w[i] = wsrc[tid + i * 256];
}

__device__ __forceinline__ void store_chunk(const Staged& s, int tid, float* s_in, float* s_w) {
#pragma unroll
  for (int c = 0; c < kCK; ++c)
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
      if (tid + j * 256 < kHalo) s_in[c * kHalo + tid + j * 256] = s.in[c * kSlots + j];
#pragma unroll
  for (int i = 0; i < kStageW; ++i) s_w[tid + i * 256] = s.w[i];
}

__global__ __launch_bounds__(256) void conv3x3x3_mfma_kernel(ConvArgs a) {
  __shared__ float s_in[kCK * kHalo];
  __shared__ float s_w[kKK * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int xb = (int)(blockIdx.x % (unsigned)a.nb2), cb = (int)(blockIdx.x / (unsigned)a.nb2);
  const int x0 = xb * kT2, y0 = blockIdx.y * kT1, z0 = blockIdx.z * kT0;
  const int zl = wave >> 1, yl = (wave & 1) * 2;  // the wave's d0 plane and the first of its two d1 rows
  f32x16 acc[2];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rs][r] = 0.f;
  const float* wp = a.wpack + (size_t)cb * a.n_chunks * (kKK * 32);
  const float* pin = s_in + h * kHalo + (zl * kH1 + yl) * kH2 + col;  // lane half h takes the odd channel of a pair
  const float* pw = s_w + h * 32 + col;
  HaloMap hm;
  map_halo(a, tid, x0, y0, z0, hm);
  Staged st;
  load_chunk(a, wp, 0, tid, hm, st);
  for (int ch = 0; ch < a.n_chunks; ++ch) {
    store_chunk(st, tid, s_in, s_w);
    __syncthreads();
    if (ch + 1 < a.n_chunks) load_chunk(a, wp, ch + 1, tid, hm, st);
#pragma unroll
    for (int cp = 0; cp < kCK / 2; ++cp) {
      f32x16 part[2];  // the 54 products of one channel pair start from zero: chains of 54, not of 27 C_in
#pragma unroll
      for (int rs = 0; rs < 2; ++rs)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[rs][r] = 0.f;
#pragma unroll
      for (int tap = 0; tap < kTaps; ++tap) {
        const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
        const float b0 = pin[cp * 2 * kHalo + (dz * kH1 + dy) * kH2 + dx];
        const float b1 = pin[cp * 2 * kHalo + (dz * kH1 + dy + 1) * kH2 + dx];
        const float wv = pw[(cp * kTaps + tap) * 2 * 32];
        part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, b0, part[0], 0, 0, 0);
        part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, b1, part[1], 0, 0, 0);
      }
      acc[0] += part[0];
      acc[1] += part[1];
    }
    __syncthreads();
  }
  const int x = x0 + col, z = z0 + zl;
  if (x >= a.D2 || z >= a.D0) return;
  float bias[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bias[r] = a.bias[min(cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, a.c_out - 1)];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs) {
    const int y = y0 + yl + rs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;  // the 32x32 C/D map: row of register r in lane half h
      if (y < a.D1 && co < a.c_out) a.out[(((size_t)co * a.D0 + z) * a.D1 + y) * a.D2 + x] = acc[rs][r] + bias[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ max-pool
__global__ __launch_bounds__(256) void maxpool3d_kernel(const float* x, float* y, int C, int D0, int D1, int D2) {
  const int O0 = D0 >> 1, O1 = D1 >> 1, O2 = D2 >> 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)C * O0 * O1 * O2) return;
  const int xo = (int)(i % O2), yo = (int)((i / O2) % O1);
  const size_t cz = i / ((size_t)O2 * O1);
  const int zo = (int)(cz % O0), c = (int)(cz / O0);
  const float* p = x + (((size_t)c * D0 + 2 * zo) * D1 + 2 * yo) * D2 + 2 * xo;
  const size_t sy = (size_t)D2, sz = (size_t)D1 * D2;
  const float a = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[sy], p[sy + 1]));
  const float b = fmaxf(fmaxf(p[sz], p[sz + 1]), fmaxf(p[sz + sy], p[sz + sy + 1]));
  y[i] = fmaxf(a, b);
}

// p[0 .. 8] of voxel i of logits [9][n]: softmax over channels 0 .. 7 and sigmoid of channel 8, in float64
__device__ __forceinline__ void head_of(const float* logits, size_t n, size_t i, double* p) {
  double m = -INFINITY, sum = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    p[c] = (double)logits[(size_t)c * n + i];
    m = fmax(m, p[c]);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    p[c] = exp(p[c] - m);
    sum += p[c];
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) p[c] = p[c] / sum;
  p[8] = 1.0 / (1.0 + exp(-(double)logits[8 * n + i]));
}

// logits [9][n] -> softmax over channels 0 .. 7 and sigmoid of channel 8, evaluated in float64 and rounded once
__global__ __launch_bounds__(256) void head_kernel(const float* logits, float* prob, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double p[9];
  head_of(logits, n, i, p);
#pragma unroll
  for (int c = 0; c < 9; ++c) prob[(size_t)c * n + i] = (float)p[c];
}

// out [c_out][D] = conv(cat(src1 [c1], src2 [c_in - c1] (upsampled when ups))) + bias
void launch_conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, const Dims& D, float* out) {
  const Dims E = ups ? D.halved_up() : D;
  ConvArgs a;
  a.src1 = src1; a.src2 = src2; a.c1 = c1; a.c2 = l.c_in - c1; a.ups = ups ? 1 : 0;
  a.D0 = D.d[0]; a.D1 = D.d[1]; a.D2 = D.d[2]; a.E0 = E.d[0]; a.E1 = E.d[1]; a.E2 = E.d[2];
  a.wpack = l.wpack; a.bias = l.bias; a.out = out; a.c_out = l.c_out; a.n_chunks = l.n_chunks;
  a.nb2 = (D.d[2] + kT2 - 1) / kT2;
  const dim3 grid((unsigned)a.nb2 * (unsigned)((l.c_out + 31) / 32), (unsigned)((D.d[1] + kT1 - 1) / kT1), (unsigned)((D.d[0] + kT0 - 1) / kT0));
  hipLaunchKernelGGL(conv3x3x3_mfma_kernel, grid, dim3(256), 0, nullptr, a);
}

void launch_maxpool(const float* x, float* y, int C, const Dims& D) {
  const size_t n = (size_t)C * D.shifted(1).voxels();
  if (n) hipLaunchKernelGGL(maxpool3d_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, x, y, C, D.d[0], D.d[1], D.d[2]);
}
