// unet_common.inc -- what speedup_net.hip (2-D) and segment_net.hip (3-D) share of the FlexUNet: the instance norm, the packing of
// the weights into the order the MFMA convolutions stage them in, the plan of the layers in the state dict's order, the buffers and
// launches of one forward pass, and the plumbing of a call's runner (device memory, the dry planning mode, the report).
// Included inside each file's unnamed namespace, after hip_host.hpp, <chrono> and the file's `constexpr int kTaps` (9 or 27: the taps
// of a convolution).  Each file keeps its own convolution and max-pool kernels and gives its Runner `conv` and `maxpool`, and a Dims
// type (the extent of a tensor without its channels) with voxels(), shifted(s) and halved_up().

using mcgpu::CallDevice;
using mcgpu::Stage;
using mcgpu::blocks_of;
using mcgpu::refuse;

#include "fixed_sum.inc"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kCK = 8;             // input channels per K chunk
constexpr int kKK = kCK * kTaps;   // K of a chunk

// ------------------------------------------------------------------------------------------------- instance norm + LeakyReLU
// Sum and sum of squares per channel in float64, over fixed segments and a fixed tree (no atomics: the same input gives the same
// bytes): four chains per thread, (0 + 1) + (2 + 3), the 256-wide tree, then the segments folded in order by one thread.  The
// normalisation is applied in float64 and rounded once.
constexpr int kMaxSegments = 64;
constexpr size_t kSegmentLength = 16384;

int segments_of(size_t n) { return (int)std::min<size_t>(kMaxSegments, (n + kSegmentLength - 1) / kSegmentLength); }

// segment s of S over n elements: [lo, hi)
struct Segment { size_t lo, hi; };
__device__ __forceinline__ Segment segment_of(size_t n, int S, int s) {
  const size_t seg = (n + S - 1) / S, lo = (size_t)s * seg;
  return {lo, min(lo + seg, n)};
}

// part[c][s] = (sum, sum of squares) of segment s of channel c, in float64 and in a fixed order
__global__ __launch_bounds__(256) void stats_kernel(const float* x, size_t hw, int S, double2* part) {
  const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const Segment g = segment_of(hw, S, s);
  const float* p = x + (size_t)c * hw;
  double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};  // four chains: four loads in flight, the order still fixed
  size_t i = g.lo + tid;
  for (; i + 768 < g.hi; i += 1024) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = p[i + 256 * k];
      sum[k] += v;
      sq[k] += v * v;
    }
  }
  for (; i < g.hi; i += 256) {
    const double v = p[i];
    sum[0] += v;
    sq[0] += v * v;
  }
  const Sums<2> total = block_tree(Sums<2>{{(sum[0] + sum[1]) + (sum[2] + sum[3]), (sq[0] + sq[1]) + (sq[2] + sq[3])}});
  if (tid == 0) part[(size_t)c * S + s] = make_double2(total.v[0], total.v[1]);
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

// ----------------------------------------------------------------------------------------------------------------- weights
// w [c_out][c_in][Taps] -> the staging order of the MFMA convolutions: per block of `ncol` output channels and chunk,
// [channel pair][tap][channel of the pair][output channel], zero where the channel does not exist
template <int Taps>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* w, float* wpack, int c_in, int c_out, int n_chunks, int ncol, size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int co_local = (int)(e % ncol);
  size_t r = e / ncol;
  const int kk = (int)(r % (kCK * Taps));
  r /= kCK * Taps;
  const int ch = (int)(r % n_chunks), cb = (int)(r / n_chunks);
  const int hh = kk & 1, tap = (kk >> 1) % Taps, cp = (kk >> 1) / Taps;
  const int ci = ch * kCK + cp * 2 + hh, co = cb * ncol + co_local;
  wpack[e] = (ci < c_in && co < c_out) ? w[((size_t)co * c_in + ci) * Taps + tap] : 0.f;
}

struct ConvLayer {
  int c_in = 0, c_out = 0;
  size_t w_off = 0, b_off = 0;  // in the flat weights
  int nb = 1, n_chunks = 0;     // nb: blocks of 32 output channels per workgroup
  float* wpack = nullptr;
  const float* bias = nullptr;
  size_t pack_floats() const { return (size_t)((c_out + 32 * nb - 1) / (32 * nb)) * n_chunks * kKK * 32 * nb; }
};

ConvLayer conv_layer(int c_in, int c_out, size_t& cursor, int nb = 1) {
  ConvLayer l;
  l.c_in = c_in;
  l.c_out = c_out;
  l.w_off = cursor;
  cursor += (size_t)c_out * c_in * kTaps;
  l.b_off = cursor;
  cursor += (size_t)c_out;
  l.nb = nb;
  l.n_chunks = (c_in + kCK - 1) / kCK;
  return l;
}

// the convolutions of one FlexUNet in the state dict's order: init, final, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0;
// f = [init, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0, final]
struct NetLayers {
  int in_channels, L;
  std::vector<int> skip_c;  // channels of out_0 .. out_L
  std::vector<int> dec_c;   // channels of dec_i's output, by level
  ConvLayer init, final;
  std::vector<ConvLayer> enc, dec;  // [2 i], [2 i + 1] of level i
  NetLayers(int in_channels_, int levels, const int* f, int n_classes, size_t& cursor)
      : in_channels(in_channels_), L(levels), skip_c(levels + 1), dec_c(levels), enc(2 * levels), dec(2 * levels) {
    skip_c[0] = f[0];
    for (int i = 0; i < L; ++i) skip_c[i + 1] = f[1 + i];
    for (int j = 0; j < L; ++j) dec_c[L - 1 - j] = f[1 + L + j];
    init = conv_layer(in_channels, f[0], cursor);
    final = conv_layer(f[2 * L + 1], n_classes, cursor);
    for (int i = 0; i < L; ++i) {
      enc[2 * i] = conv_layer(skip_c[i], skip_c[i + 1], cursor);
      enc[2 * i + 1] = conv_layer(skip_c[i + 1], skip_c[i + 1], cursor);
    }
    for (int i = L - 1; i >= 0; --i) {
      const int below = i == L - 1 ? skip_c[L] : dec_c[i + 1];
      dec[2 * i] = conv_layer(skip_c[i] + below, dec_c[i], cursor);
      dec[2 * i + 1] = conv_layer(dec_c[i], dec_c[i], cursor);
    }
  }
  template <class F>
  void each(F f) {
    f(init);
    f(final);
    for (auto& l : enc) f(l);
    for (auto& l : dec) f(l);
  }
  int widest() const {
    int w = 1;
    for (int c : skip_c) w = std::max(w, c);
    for (int c : dec_c) w = std::max(w, c);
    return w;
  }
};

// -------------------------------------------------------------------------------------------------------------------- host
// Device memory, report and shared launches of one call.  With `dry` nothing touches the device: alloc_bytes() only adds up what the
// call would hold.
template <class Report>
struct RunnerBase {
  CallDevice dev;
  Report rep;
  bool dry = false;
  size_t planned = 0;
  double2* d_part = nullptr;  // statistics of the widest layer

  RunnerBase() { memset(&rep, 0, sizeof rep); }
  void init(int device, int channels) {
    if (!dry) {
      HIP_TRY(hipSetDevice(device));
      dev.events();
    }
    d_part = (double2*)alloc_bytes((size_t)std::max(channels, 1) * kMaxSegments * sizeof(double2), true);
  }
  void* alloc_bytes(size_t bytes, bool zero) {
    bytes = std::max<size_t>(bytes, 4);
    if (dry) {
      planned += bytes;
      return nullptr;
    }
    return zero ? dev.alloc_zeroed<char>(bytes) : dev.alloc<char>(bytes);
  }
  float* alloc(size_t floats) { return (float*)alloc_bytes(floats * sizeof(float), true); }
  template <class T>
  T* upload(const T* host, size_t n) {
    T* p = (T*)alloc_bytes(n * sizeof(T), false);
    if (!dry) HIP_TRY(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }

  void pack(ConvLayer& l, const float* d_weights) {
    const size_t total = l.pack_floats();
    l.wpack = (float*)alloc_bytes(total * sizeof(float), false);
    if (dry) return;
    l.bias = d_weights + l.b_off;
    hipLaunchKernelGGL(pack_weights_kernel<kTaps>, dim3(blocks_of(total)), dim3(256), 0, nullptr, d_weights + l.w_off, l.wpack, l.c_in, l.c_out, l.n_chunks,
                       32 * l.nb, total);
  }
  void stats(const float* x, int C, size_t n, double2* part) {
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)segments_of(n), (unsigned)C), dim3(256), 0, nullptr, x, n, segments_of(n), part);
  }
  void norm_lrelu(const float* x, float* y, int C, size_t n) {
    Stage st(dev, rep.ms_norm);
    stats(x, C, n, d_part);
    hipLaunchKernelGGL(norm_lrelu_kernel, dim3(blocks_of(n), (unsigned)C), dim3(256), 0, nullptr, x, y, n, segments_of(n), d_part);
    st.done();
  }
};

template <class Report>
void finish(RunnerBase<Report>& R, const std::chrono::steady_clock::time_point& t0, Report* report) {
  R.rep.peak_device_bytes = R.dev.peak;
  R.rep.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (report) *report = R.rep;
}

// One FlexUNet at one input extent: its buffers, made once, and the launches of a forward pass
template <class Runner, class Dims>
struct NetPass {
  NetLayers& net;
  Runner& run;
  Dims P;
  std::vector<float*> skip, pooled, enc_a, dec_a, dec_b;
  float* out = nullptr;
  NetPass(NetLayers& n, Runner& r, const Dims& p) : net(n), run(r), P(p) {
    const int L = net.L;
    skip.resize(L + 1); pooled.resize(L); enc_a.resize(L); dec_a.resize(L); dec_b.resize(L);
    skip[0] = run.alloc((size_t)net.skip_c[0] * P.voxels());
    for (int i = 0; i < L; ++i) {
      const size_t below = P.shifted(i + 1).voxels(), here = P.shifted(i).voxels();
      pooled[i] = run.alloc((size_t)net.skip_c[i] * below);
      enc_a[i] = run.alloc((size_t)net.skip_c[i + 1] * below);
      skip[i + 1] = run.alloc((size_t)net.skip_c[i + 1] * below);
      dec_a[i] = run.alloc((size_t)net.dec_c[i] * here);
      dec_b[i] = run.alloc((size_t)net.dec_c[i] * here);
    }
    out = run.alloc((size_t)net.final.c_out * P.voxels());
  }
  const float* forward(const float* x) {
    const int L = net.L;
    run.conv(net.init, x, net.in_channels, nullptr, 0, P, skip[0]);
    for (int i = 0; i < L; ++i) {
      const Dims D = P.shifted(i + 1);
      const int c = net.skip_c[i + 1];
      run.maxpool(skip[i], pooled[i], net.skip_c[i], P.shifted(i));
      run.conv(net.enc[2 * i], pooled[i], net.skip_c[i], nullptr, 0, D, enc_a[i]);
      run.norm_lrelu(enc_a[i], enc_a[i], c, D.voxels());
      run.conv(net.enc[2 * i + 1], enc_a[i], c, nullptr, 0, D, skip[i + 1]);
      run.norm_lrelu(skip[i + 1], skip[i + 1], c, D.voxels());
    }
    const float* cur = skip[L];
    for (int i = L - 1; i >= 0; --i) {
      const Dims D = P.shifted(i);
      const int c = net.dec_c[i];
      run.conv(net.dec[2 * i], skip[i], net.skip_c[i], cur, 1, D, dec_a[i]);
      run.norm_lrelu(dec_a[i], dec_a[i], c, D.voxels());
      run.conv(net.dec[2 * i + 1], dec_a[i], c, nullptr, 0, D, dec_b[i]);
      run.norm_lrelu(dec_b[i], dec_b[i], c, D.voxels());
      cur = dec_b[i];
    }
    run.conv(net.final, cur, net.final.c_in, nullptr, 0, P, out);
    return out;
  }
};

// The three operators both nets have, each alone for mcgpu_*_stage: `a` is the stage's arguments, D the extent of a.in
template <class Runner, class Args, class Dims>
void stage_conv(Runner& R, const Args& a, const Dims& D, int nb = 1) {
  const Dims E = a.upsample ? D.halved_up() : D;
  const size_t n = D.voxels();
  size_t cursor = 0;
  ConvLayer l = conv_layer(a.c1 + a.c2, a.c_out, cursor, nb);
  std::vector<float> flat(cursor);
  memcpy(flat.data() + l.w_off, a.weight, (size_t)l.c_out * l.c_in * kTaps * sizeof(float));
  memcpy(flat.data() + l.b_off, a.bias, (size_t)l.c_out * sizeof(float));
  const float* d_weights = R.upload(flat.data(), flat.size());
  R.pack(l, d_weights);
  const float* d_in = R.upload(a.in, (size_t)a.c1 * n);
  const float* d_in2 = a.c2 ? R.upload(a.in2, (size_t)a.c2 * E.voxels()) : nullptr;
  float* d_out = R.alloc((size_t)a.c_out * n);
  R.conv(l, d_in, a.c1, d_in2, a.upsample, D, d_out);
  HIP_TRY(hipMemcpy(a.out, d_out, (size_t)a.c_out * n * 4, hipMemcpyDeviceToHost));
}

template <class Runner, class Args>
void stage_norm_lrelu(Runner& R, const Args& a, size_t n) {
  const float* d_in = R.upload(a.in, (size_t)a.c1 * n);
  float* d_out = R.alloc((size_t)a.c1 * n);
  R.norm_lrelu(d_in, d_out, a.c1, n);
  HIP_TRY(hipMemcpy(a.out, d_out, (size_t)a.c1 * n * 4, hipMemcpyDeviceToHost));
}

template <class Runner, class Args, class Dims>
void stage_maxpool(Runner& R, const Args& a, const Dims& D) {
  const size_t n_out = (size_t)a.c1 * D.shifted(1).voxels();
  const float* d_in = R.upload(a.in, (size_t)a.c1 * D.voxels());
  float* d_out = R.alloc(n_out);
  R.maxpool(d_in, d_out, a.c1, D);
  if (n_out) HIP_TRY(hipMemcpy(a.out, d_out, n_out * 4, hipMemcpyDeviceToHost));
}
