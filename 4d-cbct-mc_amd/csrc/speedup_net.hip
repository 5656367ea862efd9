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
//   The convolution, the max-pool, the preprocessing and the two heads stand in speedup_conv.inc, which speedup_train.hip (the
//     backward half and the trainer) includes too; the sampler and the entry points of inference stand here.
// One projection at a time (the reference runs batch size 1 per sample in effect: instance norm keeps samples independent); the
// buffers of one projection are allocated once per call.  No graphs.
#include <chrono>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

constexpr int kTaps = 9;  // 3 x 3: what unet_common.inc sizes a K chunk and counts the weights with
#include "unet_common.inc"
#include "speedup_conv.inc"  // the convolution, the small kernels of the forward pass and their launches: shared with speedup_train.hip

#include "philox_normal.inc"  // philox10, standard_normal: shared with the samplers of primary_project.hip

// sample = mean + sqrt(variance) z; with mean == nullptr: z alone
__global__ __launch_bounds__(256) void sample_kernel(const float* mean, const float* variance, float* out, int W, size_t hw, unsigned projection,
                                                     unsigned long long seed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const float z = standard_normal((int)(i % W), (int)(i / W), projection, seed);
  out[i] = mean ? mean[i] + sqrtf(variance[i]) * z : z;
}

// -------------------------------------------------------------------------------------------------------------------- host
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
    launch_conv(l, src1, c1, src2, ups, D, out);
    st.done();
  }
  void maxpool(const float* x, float* y, int C, const Dims& D) {
    Stage st(dev, rep.ms_other);
    launch_maxpool(x, y, C, D);
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
