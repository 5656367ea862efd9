// segment_net.hip -- the reference's CT segmentation network (cbctmc/segmentation/segmenter.py: MCSegmenter around a 3-D FlexUNet),
// inferred patch by patch in float32, stitched and thresholded on the device.
//
// The network.  FlexUNet(1 channel, 9 classes, L levels, filters [init, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0, final]); every
// convolution 3 x 3 x 3 with ZERO padding and bias (the 2-D sibling of speedup_net.hip pads by replication; this one does not):
//   out_0 = init_conv(x)                                                     1 -> init, full size, no norm
//   out_{i+1} = enc_i(out_i), i = 0 .. L-1:  max-pool 2 x 2 x 2, then twice [conv -> instance norm -> LeakyReLU(0.01)]
//   dec_i, i = L-1 .. 0:  cat([out_i, nearest-upsample x 2 of the running tensor]), then twice [conv -> norm -> LeakyReLU]
//   final_conv                                                               final -> 9, no norm
// Instance norm: per channel over the volume, biased variance, eps 1e-5, no affine parameters.
// The procedure.  The image is rescaled [in_min, in_max] -> [out_min, out_max] and clipped, in float32; where an axis is shorter than
// the patch it is padded with 0.0 (left = pad / 2).  Patch starts per axis: min(i s, N - P) for i s in range(0, N - P + s + 1, s), all
// combinations with the last axis fastest.  Per patch: logits -> softmax over channels 0 .. 7, sigmoid on channel 8.  Stitching keeps
// per voxel the first value k, the float32 sum of (value - k) and the count n; mean = k + sum / n.  Channel 8 becomes mean > 0.5,
// channels 0 .. 7 the one-hot of their argmax (first maximum wins).  The reference runs the convolutions in float16 under autocast;
// this is float32 throughout.
// A start that the rule gives m times is inferred once and stitched m times in a row at its first place in the order: the network is
// deterministic, so the values are those of the m runs; k is unchanged (the order of first arrivals is), only the order of the float32
// sum differs from the reference's where patches overlap, and nothing differs where they do not (value - k = 0).
//
// Tensors are [C][d0][d1][d2], d2 fastest (the image's x, y, z as torch sees the reference's [x, y, z] array).  All offsets are 64-bit.
//
// The convolution, the max-pool and the head live in segment_conv.inc, which segment_train.hip (training) includes too.
// conv3x3x3_mfma_kernel: an implicit GEMM on v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate), K = 27 C_in, on the plan of
//   conv3x3_mfma_kernel in speedup_net.hip.  The MFMA tile is transposed: rows = 32 output channels, columns = 32 voxels along d2, so a
//   lane's accumulators are one voxel of 16 channels and a store instruction writes 32 consecutive voxels.
//   The tile: a workgroup of 4 waves owns 2 (d0) x 4 (d1) x 32 (d2) voxels and 32 output channels (more output channels: more
//   workgroups); a wave owns two d1-neighbours, so one weight read feeds two MFMAs.  K runs in chunks of 8 input channels: the
//   4 x 6 x 34 halo of the chunk is staged in LDS, positions outside the tensor masked to zero (= zero padding), read from up to two
//   channel-concatenated sources, the second optionally through the x 2 nearest upsample (>> 1 on all three axes) -- neither the
//   concatenated nor the upsampled tensor exists in memory.  The global loads of chunk k + 1 go into registers before the MFMAs of
//   chunk k and to LDS after them.  Weights are packed once per call (pack_weights_kernel): per block of 32 output channels and chunk,
//   [channel pair][tap][channel of the pair][output channel], zero where a channel does not exist.  Input channels past C_in are
//   staged as zeros, output channels past C_out are not stored.  NO layer takes a VALU kernel: init (1 -> F) and final (F -> 9) run
//   here with their padding.
//   Summation: the 54 products of a channel pair (27 taps x 2 channels) run as one fma chain from zero and the pairs are added up
//   in order.  One chain over all 27 C_in products (864 at 32 channels) put the whole network 2 - 3.2 x the float32 CPU error of torch
//   away from float64; with the pairs it is below that error (profiles/segment_ab.md).  The cost is 32 v_add_f32 per 54 MFMAs.
//   Resources (compiler's report, gfx950): 196 VGPRs + 32 AGPRs, no scratch, LDS 53,760 B per workgroup (halo 8 x 816 floats =
//   26,112 B, weights 216 x 32 floats = 27,648 B): the registers hold 2 waves per SIMD, so 2 workgroups are resident per CU (the
//   160 KiB of LDS would hold 3).  Tried and rejected: staging the halo as one flat run of 8 x 816 floats over the threads (the
//   compiler keeps a 64-bit offset and a mask per element across the chunks: 245 VGPRs, 95 spilled SGPRs, 1 wave per SIMD); now a
//   thread keeps the same 4 halo positions in every channel and one 32-bit offset per position and source.
//   Rejected without a measurement, on arithmetic alone: 64 output channels per workgroup (the reference has 32 everywhere: half of
//   every MFMA would multiply zeros); a 2 x 2 x 64 tile (halo 4 x 4 x 66 = 1056 floats per channel against 816 for the same 256
//   voxels); chunks of 16 channels (107 KB of LDS: one workgroup per CU).
// Instance norm (stats_kernel + norm_lrelu_kernel: float64 sums over fixed segments and a fixed tree, normalised in float64, rounded
//   once; the same input gives the same bytes), the packing of the weights, the plan of the layers and the launches of a forward pass
//   are unet_common.inc's, shared with speedup_net.hip.
// maxpool3d_kernel, stage_patch_kernel (reads the image as float32 or int16, rescales, 0.0 outside the image: no padded copy of the
//   image exists), head_kernel (softmax and sigmoid evaluated in float64, rounded once), stitch_kernel (k, sum, n of the padded volume;
//   patches run one after the other on one stream: no atomics), mean_kernel, labels_kernel.
#include <chrono>
#include <memory>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

constexpr int kTaps = 27;  // 3 x 3 x 3: what unet_common.inc sizes a K chunk and counts the weights with
#include "unet_common.inc"
#include "segment_conv.inc"

// ------------------------------------------------------------------------------------------------------------- small kernels
struct Rescale { float in_min, in_span, out_min, out_span, out_max; int on; };  // on = 0: the ranges are equal, values pass

// patch [P0][P1][P2] at `start` of the padded volume = the rescaled image where it exists (padded position - left), else 0.0
template <class T>
__global__ __launch_bounds__(256) void stage_patch_kernel(const T* image, int N0, int N1, int N2, int l0, int l1, int l2, int s0, int s1, int s2, int P0,
                                                          int P1, int P2, Rescale r, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)P0 * P1 * P2) return;
  const int x = (int)(i % P2) + s2 - l2, y = (int)((i / P2) % P1) + s1 - l1, z = (int)(i / ((size_t)P2 * P1)) + s0 - l0;
  float v = 0.f;
  if (z >= 0 && z < N0 && y >= 0 && y < N1 && x >= 0 && x < N2) {
    v = (float)image[((size_t)z * N1 + y) * N2 + x];
    if (r.on) {
      v = ((v - r.in_min) * r.out_span) / r.in_span + r.out_min;
      v = fminf(fmaxf(v, r.out_min), r.out_max);
    }
  }
  out[i] = v;
}

// `times` additions of one patch [C][P0][P1][P2] at `start` into (k, sum) [C][V0][V1][V2] and count [V0][V1][V2]
__global__ __launch_bounds__(256) void stitch_kernel(const float* patch, int C, int P0, int P1, int P2, int s0, int s1, int s2, int V0, int V1, int V2,
                                                     int times, float* k, float* sum, unsigned* count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, np = (size_t)P0 * P1 * P2, nv = (size_t)V0 * V1 * V2;
  if (i >= np) return;
  const int x = (int)(i % P2) + s2, y = (int)((i / P2) % P1) + s1, z = (int)(i / ((size_t)P2 * P1)) + s0;
  const size_t g = ((size_t)z * V1 + y) * V2 + x;
  const unsigned have = count[g];
  for (int c = 0; c < C; ++c) {
    const float d = patch[(size_t)c * np + i];
    const size_t gc = (size_t)c * nv + g;
    const float first = have ? k[gc] : d;
    if (!have) k[gc] = d;
    float s = sum[gc];
    const float diff = d - first;
    for (int t = 0; t < times; ++t) s += diff;
    sum[gc] = s;
  }
  count[g] = have + (unsigned)times;
}

// mean = k + sum / n (0 where nothing arrived), written over sum
__global__ __launch_bounds__(256) void mean_kernel(const float* k, float* sum, const unsigned* count, int C, size_t nv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const unsigned n = count[i];
  for (int c = 0; c < C; ++c) {
    const size_t g = (size_t)c * nv + i;
    sum[g] = n ? k[g] + sum[g] / (float)n : 0.f;
  }
}

// mean [9][nv] -> labels: one-hot of the argmax of channels 0 .. 7 (first maximum wins), channel 8 > 0.5
__global__ __launch_bounds__(256) void labels_kernel(const float* mean, unsigned char* labels, size_t nv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  int best = 0;
  float top = mean[i];
  for (int c = 1; c < 8; ++c) {
    const float v = mean[(size_t)c * nv + i];
    if (v > top) {
      top = v;
      best = c;
    }
  }
  for (int c = 0; c < 8; ++c) labels[(size_t)c * nv + i] = c == best ? 1 : 0;
  labels[8 * nv + i] = mean[8 * nv + i] > 0.5f ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------------- host
// Launches of one call; RunnerBase's dry mode plans the buffers of mcgpu_segment_run without touching the device
struct Runner : RunnerBase<mcgpu_segment_report> {

  // out [c_out][D] = conv(cat(src1 [c1], src2 [c_in - c1] (upsampled when ups))) + bias
  void conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, const Dims& D, float* out) {
    Stage st(dev, rep.ms_conv);
    launch_conv(l, src1, c1, src2, ups, D, out);
    st.done();
  }
  void maxpool(const float* x, float* y, int C, const Dims& D) {
    Stage st(dev, rep.ms_other);
    launch_maxpool(x, y, C, D);
    st.done();
  }
  void head(const float* logits, float* prob, size_t n) {
    Stage st(dev, rep.ms_other);
    hipLaunchKernelGGL(head_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, logits, prob, n);
    st.done();
  }
  void stitch(const float* patch, int C, const Dims& P, const int* start, const Dims& V, int times, float* k, float* sum, unsigned* count) {
    Stage st(dev, rep.ms_other);
    hipLaunchKernelGGL(stitch_kernel, dim3(blocks_of(P.voxels())), dim3(256), 0, nullptr, patch, C, P.d[0], P.d[1], P.d[2], start[0], start[1], start[2],
                       V.d[0], V.d[1], V.d[2], times, k, sum, count);
    st.done();
  }
  void mean(const float* k, float* sum, const unsigned* count, int C, size_t nv) {
    Stage st(dev, rep.ms_other);
    hipLaunchKernelGGL(mean_kernel, dim3(blocks_of(nv)), dim3(256), 0, nullptr, k, sum, count, C, nv);
    st.done();
  }
  void labels(const float* mean, unsigned char* out, size_t nv) {
    Stage st(dev, rep.ms_other);
    hipLaunchKernelGGL(labels_kernel, dim3(blocks_of(nv)), dim3(256), 0, nullptr, mean, out, nv);
    st.done();
  }
};

constexpr int kMaxLevels = 8;
constexpr int kClasses = 9;

struct Patch { int start[3]; int times; };

std::string triple(const int* v) { return std::to_string(v[0]) + " x " + std::to_string(v[1]) + " x " + std::to_string(v[2]); }

// everything mcgpu_segment_run refuses from its arguments alone; fills the padded shape, the left pads and the patches in their order
void check_run(const mcgpu_segment_options& o, const void* image, const unsigned char* labels, Dims& V, int* left, std::vector<Patch>& patches,
               size_t& n_rule) {
  const char* fn = "mcgpu_segment_run";
  if (!image) refuse(fn, "image is NULL");
  if (!labels) refuse(fn, "labels is NULL");
  if (!o.weights) refuse(fn, "weights is NULL");
  if (o.image_type != MCGPU_IMAGE_INT16 && o.image_type != MCGPU_IMAGE_FLOAT32) refuse(fn, "image_type " + std::to_string(o.image_type) + ": MCGPU_IMAGE_INT16 or MCGPU_IMAGE_FLOAT32");
  for (int a = 0; a < 3; ++a)
    if (o.shape[a] < 1 || o.patch_shape[a] < 1) refuse(fn, "shape and patch_shape must be >= 1: " + triple(o.shape) + ", " + triple(o.patch_shape));
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
  int stride[3];
  for (int a = 0; a < 3; ++a) {
    const double s = (1.0 - o.patch_overlap) * o.patch_shape[a];
    if (!(s >= 1.0) || s != std::floor(s) || s > 2147483647.0)
      refuse(fn, "patch_overlap " + std::to_string(o.patch_overlap) + " gives a stride of " + std::to_string(s) + " on patch axis " + std::to_string(a) +
                     " (" + std::to_string(o.patch_shape[a]) + "): a whole number >= 1 is needed (the reference truncates silently)");
    stride[a] = (int)s;
  }
  if (o.in_max == o.in_min && !(o.in_min == o.out_min && o.in_max == o.out_max)) refuse(fn, "input_value_range is empty");
  std::vector<int> starts[3];
  for (int a = 0; a < 3; ++a) {
    V.d[a] = std::max(o.shape[a], o.patch_shape[a]);
    left[a] = (V.d[a] - o.shape[a]) / 2;
    const long long top = (long long)V.d[a] - o.patch_shape[a];
    for (long long v = 0; v < top + stride[a] + 1; v += stride[a]) starts[a].push_back((int)std::min(v, top));
  }
  if (V.voxels() > 0x7fffffffull * 64) refuse(fn, "the padded volume " + triple(V.d) + " is too large");
  n_rule = 0;
  for (int i : starts[0])
    for (int j : starts[1])
      for (int k : starts[2]) {
        ++n_rule;
        bool seen = false;
        for (auto& p : patches)
          if (p.start[0] == i && p.start[1] == j && p.start[2] == k) {
            ++p.times;
            seen = true;
            break;
          }
        if (!seen) patches.push_back({{i, j, k}, 1});
      }
}

size_t image_bytes(const mcgpu_segment_options& o) {
  return ((size_t)o.shape[0] * o.shape[1]) * o.shape[2] * (o.image_type == MCGPU_IMAGE_INT16 ? 2 : 4);
}

struct RunBuffers {
  const void* d_image = nullptr;
  const float* d_weights = nullptr;
  float *d_x = nullptr, *d_prob = nullptr, *d_k = nullptr, *d_sum = nullptr;
  unsigned* d_count = nullptr;
  unsigned char* d_labels = nullptr;
};

// every buffer of a run, in one place: made on the device, or (Runner::dry) only added up
void make_buffers(Runner& R, const mcgpu_segment_options& o, const void* image, NetLayers& net, const Dims& P, const Dims& V, RunBuffers& b,
                  std::unique_ptr<NetPass<Runner, Dims>>& pass) {
  R.init(o.device, net.widest());
  b.d_weights = R.upload(o.weights, (size_t)o.n_weights);
  net.each([&](ConvLayer& l) { R.pack(l, b.d_weights); });
  b.d_image = R.upload((const char*)image, image_bytes(o));
  b.d_x = R.alloc(P.voxels());
  pass.reset(new NetPass<Runner, Dims>(net, R, P));
  b.d_prob = R.alloc((size_t)kClasses * P.voxels());
  b.d_k = R.alloc((size_t)kClasses * V.voxels());
  b.d_sum = R.alloc((size_t)kClasses * V.voxels());
  b.d_count = (unsigned*)R.alloc_bytes(V.voxels() * sizeof(unsigned), true);
  b.d_labels = (unsigned char*)R.alloc_bytes((size_t)kClasses * V.voxels(), true);
}


}  // namespace

extern "C" int mcgpu_segment_run(const mcgpu_segment_options* caller_o, const void* image, unsigned char* labels, float* raw, mcgpu_segment_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_run";
  mcgpu_segment_options o;
  mcgpu::read_options(fn, "mcgpu_segment_options", caller_o, o);
  Dims V, P{{o.patch_shape[0], o.patch_shape[1], o.patch_shape[2]}};
  int left[3];
  std::vector<Patch> patches;
  size_t n_rule = 0;
  check_run(o, image, labels, V, left, patches, n_rule);
  const auto t0 = std::chrono::steady_clock::now();
  size_t cursor = 0;
  NetLayers net(1, o.levels, o.n_filters, o.n_classes, cursor);
  size_t needed = 0;
  {
    Runner plan;
    plan.dry = true;
    RunBuffers b;
    std::unique_ptr<NetPass<Runner, Dims>> pass;
    make_buffers(plan, o, image, net, P, V, b, pass);
    needed = plan.planned;
  }
  if (o.memory_limit_bytes && needed > o.memory_limit_bytes)
    refuse(fn, "the call needs " + std::to_string(needed) + " bytes of device memory, above the limit of " + std::to_string(o.memory_limit_bytes));
  Runner R;
  HIP_TRY(hipSetDevice(o.device));
  size_t free_bytes = 0, total_bytes = 0;
  HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
  if (needed > free_bytes)
    refuse(fn, "the call needs " + std::to_string(needed) + " bytes of device memory, the device has " + std::to_string(free_bytes) + " free");
  RunBuffers b;
  std::unique_ptr<NetPass<Runner, Dims>> pass;
  {
    const auto u0 = std::chrono::steady_clock::now();
    make_buffers(R, o, image, net, P, V, b, pass);
    HIP_TRY(hipDeviceSynchronize());
    R.rep.ms_upload += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
  }
  Rescale rs;
  rs.in_min = (float)o.in_min; rs.in_span = (float)(o.in_max - o.in_min); rs.out_min = (float)o.out_min; rs.out_span = (float)(o.out_max - o.out_min);
  rs.out_max = (float)o.out_max;
  rs.on = !(o.in_min == o.out_min && o.in_max == o.out_max);
  for (const Patch& p : patches) {
    {
      Stage st(R.dev, R.rep.ms_other);
      const dim3 grid(blocks_of(P.voxels()));
      if (o.image_type == MCGPU_IMAGE_INT16)
        hipLaunchKernelGGL(stage_patch_kernel<short>, grid, dim3(256), 0, nullptr, (const short*)b.d_image, o.shape[0], o.shape[1], o.shape[2], left[0], left[1],
                           left[2], p.start[0], p.start[1], p.start[2], P.d[0], P.d[1], P.d[2], rs, b.d_x);
      else
        hipLaunchKernelGGL(stage_patch_kernel<float>, grid, dim3(256), 0, nullptr, (const float*)b.d_image, o.shape[0], o.shape[1], o.shape[2], left[0], left[1],
                           left[2], p.start[0], p.start[1], p.start[2], P.d[0], P.d[1], P.d[2], rs, b.d_x);
      st.done();
    }
    const float* logits = pass->forward(b.d_x);
    R.head(logits, b.d_prob, P.voxels());
    R.stitch(b.d_prob, kClasses, P, p.start, V, p.times, b.d_k, b.d_sum, b.d_count);
  }
  R.mean(b.d_k, b.d_sum, b.d_count, kClasses, V.voxels());
  R.labels(b.d_sum, b.d_labels, V.voxels());
  {
    Stage st(R.dev, R.rep.ms_upload);
    HIP_TRY(hipMemcpy(labels, b.d_labels, (size_t)kClasses * V.voxels(), hipMemcpyDeviceToHost));
    if (raw) HIP_TRY(hipMemcpy(raw, b.d_sum, (size_t)kClasses * V.voxels() * 4, hipMemcpyDeviceToHost));
    st.done();
  }
  R.rep.patches_run = (unsigned long long)patches.size();
  R.rep.patches_skipped = (unsigned long long)(n_rule - patches.size());
  R.rep.planned_device_bytes = needed;
  finish(R, t0, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_segment_stage(const mcgpu_segment_options* caller_o, int stage, const mcgpu_segment_stage_args* caller_a, mcgpu_segment_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_segment_stage";
  mcgpu_segment_options o;
  mcgpu::read_options(fn, "mcgpu_segment_options", caller_o, o);
  mcgpu_segment_stage_args a;
  mcgpu::read_options(fn, "mcgpu_segment_stage_args", caller_a, a);
  if (stage < MCGPU_SEGMENT_STAGE_CONV || stage > MCGPU_SEGMENT_STAGE_FINALIZE) refuse(fn, "unknown stage " + std::to_string(stage));
  if (!a.out) refuse(fn, "out is NULL");
  if (!a.in) refuse(fn, "in is NULL");
  for (int i = 0; i < 3; ++i)
    if (a.shape[i] < 1) refuse(fn, "shape must be >= 1: " + triple(a.shape));
  const Dims D{{a.shape[0], a.shape[1], a.shape[2]}};
  const size_t n = D.voxels();
  if ((size_t)((D.d[0] + kT0 - 1) / kT0) > 65535 || (size_t)((D.d[1] + kT1 - 1) / kT1) > 65535 || n > 0x7fffffffull)
    refuse(fn, "shape " + triple(a.shape) + " is too large: at most 2^31 - 1 voxels");
  if (stage <= MCGPU_SEGMENT_STAGE_MAXPOOL || stage == MCGPU_SEGMENT_STAGE_STITCH)
    if (a.c1 < 1 || a.c1 > 65535) refuse(fn, "c1 must be 1..65535");
  if (stage == MCGPU_SEGMENT_STAGE_CONV) {
    if (a.c2 < 0 || a.c2 > 65535 || a.c_out < 1 || a.c_out > 65535) refuse(fn, "c2 must be 0..65535 and c_out 1..65535");
    if (!a.weight || !a.bias) refuse(fn, "weight or bias is NULL");
    if (a.c2 > 0 && !a.in2) refuse(fn, "in2 is NULL");
  }
  if (stage == MCGPU_SEGMENT_STAGE_NORM_LRELU && n < 2) refuse(fn, "instance norm needs at least 2 voxels");
  if (stage == MCGPU_SEGMENT_STAGE_STITCH) {
    if (a.n_patches < 1 || !a.starts) refuse(fn, "n_patches must be >= 1 and starts given");
    for (int p = 0; p < a.n_patches; ++p)
      for (int i = 0; i < 3; ++i)
        if (a.patch_shape[i] < 1 || a.starts[3 * p + i] < 0 || a.starts[3 * p + i] + a.patch_shape[i] > a.shape[i])
          refuse(fn, "patch " + std::to_string(p) + " at " + triple(a.starts + 3 * p) + " of shape " + triple(a.patch_shape) + " leaves the volume " + triple(a.shape));
  }
  const auto t0 = std::chrono::steady_clock::now();
  Runner R;
  R.init(o.device, stage == MCGPU_SEGMENT_STAGE_NORM_LRELU ? a.c1 : 1);
  switch (stage) {
    case MCGPU_SEGMENT_STAGE_CONV: stage_conv(R, a, D); break;
    case MCGPU_SEGMENT_STAGE_NORM_LRELU: stage_norm_lrelu(R, a, n); break;
    case MCGPU_SEGMENT_STAGE_MAXPOOL: stage_maxpool(R, a, D); break;
    case MCGPU_SEGMENT_STAGE_HEAD: {
      const float* d_in = R.upload(a.in, (size_t)kClasses * n);
      float* d_out = R.alloc((size_t)kClasses * n);
      R.head(d_in, d_out, n);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)kClasses * n * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_SEGMENT_STAGE_STITCH: {
      const Dims P{{a.patch_shape[0], a.patch_shape[1], a.patch_shape[2]}};
      const size_t per = (size_t)a.c1 * P.voxels();
      const float* d_in = R.upload(a.in, per * a.n_patches);
      float *d_k = R.alloc((size_t)a.c1 * n), *d_sum = R.alloc((size_t)a.c1 * n);
      unsigned* d_count = (unsigned*)R.alloc_bytes(n * sizeof(unsigned), true);
      for (int p = 0; p < a.n_patches; ++p) R.stitch(d_in + per * p, a.c1, P, a.starts + 3 * p, D, 1, d_k, d_sum, d_count);
      R.mean(d_k, d_sum, d_count, a.c1, n);
      HIP_TRY(hipMemcpy(a.out, d_sum, (size_t)a.c1 * n * 4, hipMemcpyDeviceToHost));
      break;
    }
    default: {
      const float* d_in = R.upload(a.in, (size_t)kClasses * n);
      unsigned char* d_out = (unsigned char*)R.alloc_bytes((size_t)kClasses * n, true);
      R.labels(d_in, d_out, n);
      HIP_TRY(hipMemcpy(a.out, d_out, (size_t)kClasses * n, hipMemcpyDeviceToHost));
    }
  }
  finish(R, t0, report);
  return 0;
  ABI_END
}
