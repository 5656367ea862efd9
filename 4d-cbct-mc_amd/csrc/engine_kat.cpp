// engine_kat.cpp -- C ABI of the device-side known-answer hooks of the parity tests and of the micro-benchmarks behind the
// bench line's ceilings (include/mcgpu_amd.h: mcgpu_kat_*, mcgpu_microbench).
#include "engine_internal.hpp"

using namespace mcgpu;

extern "C" {

int mcgpu_microbench(mcgpu_ctx* ctx, int kind, double* out, int n_out) {
  ABI_BEGIN
  require(ctx && ctx->has_device && out && ((kind == MCGPU_MICROBENCH_VALU_ISSUE && n_out >= 3) || ((kind == MCGPU_MICROBENCH_ATOMIC_RATE || kind == MCGPU_MICROBENCH_COPY_RATE) && n_out >= 1)), -1,
          "!!ERROR!! mcgpu_microbench: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  HIP_TRY(hipDeviceSynchronize());
  if (kind == MCGPU_MICROBENCH_VALU_ISSUE) HIP_TRY(microbench_valu_issue(ctx->dev.num_cus, out, nullptr));
  else if (kind == MCGPU_MICROBENCH_COPY_RATE) HIP_TRY(microbench_copy_rate(ctx->dev.num_cus, out, nullptr));
  else HIP_TRY(microbench_atomic_rate(out, nullptr));
  return 0;
  ABI_END
}

int mcgpu_kat_rng(mcgpu_ctx* ctx, int mode, int seed, int batch, int hpt, int n, float* out_f32) {
  ABI_BEGIN
  require(ctx && ctx->has_device && out_f32 && n > 0, -1, "!!ERROR!! mcgpu_kat_rng: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  float* d = dev.alloc<float>((size_t)n * 4);
  HIP_TRY(launch_kat_rng(mode, seed, batch, hpt, n, d, nullptr));
  HIP_TRY(hipMemcpy(out_f32, d, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_rng_streams(mcgpu_ctx* ctx, int generator, unsigned int seed, unsigned int projection, unsigned long long first_id,
                          const unsigned long long* ids, int n_ids, int n_draws, uint32_t* out_u32) {
  ABI_BEGIN
  require(ctx && ctx->has_device && out_u32 && n_ids > 0 && n_draws > 0 && (generator == 0 || generator == 1) &&
              (size_t)n_ids * (size_t)n_draws <= ((size_t)1 << 30),
          -1, "!!ERROR!! mcgpu_kat_rng_streams: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  const size_t nb = (size_t)n_ids * (size_t)n_draws * 4;
  unsigned int* d = dev.alloc<unsigned int>(nb);
  const unsigned long long* d_ids = ids ? dev.upload(ids, (size_t)n_ids) : nullptr;
  HIP_TRY(launch_kat_streams_fast(generator, seed, projection, first_id, d_ids, n_ids, n_draws, d, nullptr));
  HIP_TRY(hipMemcpy(out_u32, d, nb, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_math(mcgpu_ctx* ctx, int n, const double* x, double* out_log, double* out_exp, double* out_sin, double* out_cos) {
  ABI_BEGIN
  require(ctx && ctx->has_device && x && out_log && out_exp && out_sin && out_cos && n > 0, -1, "!!ERROR!! mcgpu_kat_math: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  const size_t nb = (size_t)n * 8;
  double* d = dev.alloc<double>(5 * nb);
  HIP_TRY(hipMemcpy(d, x, nb, hipMemcpyHostToDevice));
  HIP_TRY(launch_kat_math(n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, nullptr));
  HIP_TRY(hipMemcpy(out_log, d + n, nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_exp, d + 2 * n, nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_sin, d + 3 * n, nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_cos, d + 4 * n, nb, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_fast64(mcgpu_ctx* ctx, int n, const uint32_t* u, const double* a, const double* b, const double* c, const float* dir3, double* out8) {
  ABI_BEGIN
  require(ctx && ctx->has_device && u && a && b && c && dir3 && out8 && n > 0, -1, "!!ERROR!! mcgpu_kat_fast64: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  const size_t n8 = (size_t)n * 8, n4 = (size_t)n * 4;
  double* d_out = dev.alloc<double>(11 * n8 + n4 + 3 * n4);  // out (8 n doubles) | a | b | c | u | dir
  double *d_a = d_out + 8 * (size_t)n, *d_b = d_a + n, *d_c = d_b + n;
  unsigned int* d_u = (unsigned int*)(d_c + n);
  float* d_dir = (float*)(d_u + n);
  HIP_TRY(hipMemcpy(d_a, a, n8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_b, b, n8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_c, c, n8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_u, u, n4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_dir, dir3, 3 * n4, hipMemcpyHostToDevice));
  HIP_TRY(launch_kat_fast64(n, d_u, d_a, d_b, d_c, d_dir, d_out, nullptr));
  HIP_TRY(hipMemcpy(out8, d_out, 8 * n8, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_scatter(mcgpu_ctx* ctx, int mode, int kind, int n, unsigned int seed, unsigned int stream_key, const float* in4,
                      const unsigned long long* in_u64, const int* material, float* out4, uint32_t* out_u4) {
  ABI_BEGIN
  require(ctx && ctx->has_device && in4 && in_u64 && out4 && out_u4 && n > 0 && n <= (1 << 24), -1, "!!ERROR!! mcgpu_kat_scatter: bad argument");
  require(mode == MCGPU_MODE_FAST || mode == MCGPU_MODE_FAST_F64, -1, "!!ERROR!! mcgpu_kat_scatter: the hook exists in the FAST arithmetics only");
  require(kind == MCGPU_KAT_ROTATE || kind == MCGPU_KAT_RAYLEIGH || kind == MCGPU_KAT_COMPTON, -1, "!!ERROR!! mcgpu_kat_scatter: unknown kind");
  require(kind != MCGPU_KAT_ROTATE || mode == MCGPU_MODE_FAST, -1, "!!ERROR!! mcgpu_kat_scatter: the rotation of MCGPU_MODE_FAST_F64 is mcgpu_kat_fast64's");
  const DeviceModel& D = ctx->dev;
  std::vector<int> mc((size_t)n, 0);
  if (kind != MCGPU_KAT_ROTATE) {
    // what the kernel indexes its tables with is checked here: a material the model holds, an energy inside the tables
    require(material != nullptr, -1, "!!ERROR!! mcgpu_kat_scatter: no materials");
    const float e0 = ctx->host.mat.e0, ide = ctx->host.mat.ide, top = (float)(ctx->host.mat.num_values - 1);
    for (int i = 0; i < n; ++i) {
      require(material[i] >= 0 && material[i] < kMaxMaterials && D.compact_of[material[i]] >= 0, -2,
              "!!ERROR!! mcgpu_kat_scatter: a material that no voxel of the context's geometry holds");
      mc[(size_t)i] = D.compact_of[material[i]];
      const float t = (in4[4 * (size_t)i + 3] - e0) * ide;
      require(t >= 0.0f && t < top, -2, "!!ERROR!! mcgpu_kat_scatter: an energy outside the cross-section tables");
    }
  }
  HIP_TRY(hipSetDevice(D.device_id));
  TrackArgs A = make_args(*ctx, 0);
  A.dose_flags = 0;
  CallDevice dev;
  const size_t n16 = (size_t)n * 16;
  float* d_in = dev.upload(in4, (size_t)n * 4);
  const unsigned long long* d_u64 = dev.upload(in_u64, (size_t)n);
  const int* d_mc = dev.upload(mc.data(), (size_t)n);
  float* d_out = dev.alloc_zeroed<float>(n16);
  unsigned int* d_out_u = dev.alloc_zeroed<unsigned int>(n16);
  HIP_TRY((mode == MCGPU_MODE_FAST_F64 ? launch_kat_scatter_fast64 : launch_kat_scatter_fast)(A, kind, n, seed, stream_key, d_in, d_u64, d_mc, d_out, d_out_u, nullptr));
  HIP_TRY(hipMemcpy(out4, d_out, n16, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_u4, d_out_u, n16, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_history(mcgpu_ctx* ctx, int mode, int kind, int projection, int n, unsigned int seed, const float* in8, const unsigned long long* in_u64,
                      float* out8, uint32_t* out_u8) {
  ABI_BEGIN
  require(ctx && ctx->has_device && out8 && out_u8 && n > 0 && n <= (1 << 24), -1, "!!ERROR!! mcgpu_kat_history: bad argument");
  require(mode == MCGPU_MODE_FAST || mode == MCGPU_MODE_FAST_F64, -1, "!!ERROR!! mcgpu_kat_history: the hook exists in the FAST arithmetics only");
  require(kind == MCGPU_KAT_SOURCE || kind == MCGPU_KAT_TALLY || kind == MCGPU_KAT_HOP, -1, "!!ERROR!! mcgpu_kat_history: unknown kind");
  require(projection >= 0 && projection < ctx->host.cfg.num_projections, -1, "!!ERROR!! mcgpu_kat_history: a projection outside the context");
  require((kind == MCGPU_KAT_SOURCE || in8 != nullptr) && (kind == MCGPU_KAT_TALLY || in_u64 != nullptr), -1, "!!ERROR!! mcgpu_kat_history: an input of this kind is missing");
  const DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  TrackArgs A = make_args(*ctx, projection);
  A.dose_flags = 0;
  A.first = 0;  // the id an item passes is its stream's id
  A.seed = (int)seed;
  // what the kernel indexes its tables with is checked here.  None of the three kinds indexes anything by the photon's position (the
  // exterior is crossed analytically, the detector is a plane); positions and directions only have to be numbers.
  const float e0 = ctx->host.mat.e0, ide = ctx->host.mat.ide, top = (float)(ctx->host.mat.num_values - 1);
  auto in_tables = [&](float e) { const float t = (e - e0) * ide; return t >= 0.0f && t < top; };
  if (kind == MCGPU_KAT_SOURCE) {  // every energy the spectrum can hand out (below its last edge): the record of its bin
    const Spectrum& S = ctx->host.spectrum;
    require(S.num_bins > 0 && in_tables(S.espc[0]) && (S.espc[S.num_bins] - e0) * ide <= top, -2,
            "!!ERROR!! mcgpu_kat_history: a spectrum energy outside the cross-section tables");
  } else {
    require(kind != MCGPU_KAT_HOP || (A.has_exterior & 2) != 0, -2, "!!ERROR!! mcgpu_kat_history: the context's geometry has no homogeneous exterior to hop across");
    for (int i = 0; i < n; ++i) {
      const float* p = in8 + 8 * (size_t)i;
      for (int k = 0; k < 7; ++k) require(std::isfinite(p[k]), -2, "!!ERROR!! mcgpu_kat_history: an input that is not a number");
      if (kind == MCGPU_KAT_HOP) require(in_tables(p[6]), -2, "!!ERROR!! mcgpu_kat_history: an energy outside the cross-section tables");
      else  // the tally looks nothing up by energy: its value must fit the 32-bit word the kernels hand to tally_score
        require(p[6] >= 0.0f && p[6] < 4.0e7f && p[7] >= 0.0f && p[7] <= 3.0f && p[7] == (float)(int)p[7], -2,
                "!!ERROR!! mcgpu_kat_history: a tally energy or scatter state out of range");
    }
  }
  CallDevice dev;
  const size_t n32 = (size_t)n * 32;
  const float* d_in = in8 ? dev.upload(in8, (size_t)n * 8) : nullptr;
  const unsigned long long* d_u64 = in_u64 ? dev.upload(in_u64, (size_t)n) : nullptr;
  float* d_out = dev.alloc_zeroed<float>(n32);
  unsigned int* d_out_u = dev.alloc_zeroed<unsigned int>(n32);
  HIP_TRY((mode == MCGPU_MODE_FAST_F64 ? launch_kat_history_fast64 : launch_kat_history_fast)(A, kind, n, d_in, d_u64, d_out, d_out_u, nullptr));
  HIP_TRY(hipMemcpy(out8, d_out, n32, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_u8, d_out_u, n32, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_flight(mcgpu_ctx* ctx, int mode, int kind, int projection, int n, int max_steps, unsigned int seed, const float* in8,
                     const unsigned long long* in_u64, uint32_t* out_u32) {
  ABI_BEGIN
  require(ctx && ctx->has_device && in8 && out_u32 && n > 0 && n <= (1 << 20), -1, "!!ERROR!! mcgpu_kat_flight: bad argument");
  require(mode == MCGPU_MODE_FAST || mode == MCGPU_MODE_FAST_F64, -1, "!!ERROR!! mcgpu_kat_flight: the hook exists in the FAST arithmetics only");
  require(kind == MCGPU_KAT_LOOKUP || kind == MCGPU_KAT_FLIGHT, -1, "!!ERROR!! mcgpu_kat_flight: unknown kind");
  require(projection >= 0 && projection < ctx->host.cfg.num_projections, -1, "!!ERROR!! mcgpu_kat_flight: a projection outside the context");
  const bool flight = kind == MCGPU_KAT_FLIGHT;
  if (flight) {
    require(in_u64 != nullptr, -1, "!!ERROR!! mcgpu_kat_flight: an input of this kind is missing");
    require(max_steps >= 1 && max_steps <= 32 && (long long)n * max_steps <= (1LL << 22), -1, "!!ERROR!! mcgpu_kat_flight: step count out of range");
  }
  // what the kernel indexes its tables with is checked here, before any HIP call.  A position only has to be a number: the flight step
  // clamps it to the volume before it indexes anything.  The step count is bounded by the argument.
  const float e0 = ctx->host.mat.e0, ide = ctx->host.mat.ide, top = (float)(ctx->host.mat.num_values - 1);
  for (int i = 0; i < n; ++i) {
    const float* p = in8 + 8 * (size_t)i;
    for (int k = 0; k < (flight ? 7 : 3); ++k) require(std::isfinite(p[k]), -2, "!!ERROR!! mcgpu_kat_flight: an input that is not a number");
    if (flight) {
      require(p[3] != 0.0f || p[4] != 0.0f || p[5] != 0.0f, -2, "!!ERROR!! mcgpu_kat_flight: a direction of length zero");
      const float t = (p[6] - e0) * ide;
      require(t >= 0.0f && t < top, -2, "!!ERROR!! mcgpu_kat_flight: an energy outside the cross-section tables");
    }
  }
  const DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  TrackArgs A = make_args(*ctx, projection);
  A.dose_flags = 0;
  A.first = 0;  // the id an item passes is its stream's id
  A.seed = (int)seed;
  CallDevice dev;
  const size_t words = (size_t)n * 8 * (flight ? (size_t)max_steps + 1 : 1);
  const float* d_in = dev.upload(in8, (size_t)n * 8);
  const unsigned long long* d_u64 = in_u64 ? dev.upload(in_u64, (size_t)n) : nullptr;
  unsigned int* d_out = dev.alloc_zeroed<unsigned int>(words * 4);
  HIP_TRY((mode == MCGPU_MODE_FAST_F64 ? launch_kat_flight_fast64 : launch_kat_flight_fast)(A, kind, n, flight ? max_steps : 0, d_in, d_u64, d_out, nullptr));
  HIP_TRY(hipMemcpy(out_u32, d_out, words * 4, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_f32(mcgpu_ctx* ctx, int op, int n, const float* a, const float* b, float* inout) {
  ABI_BEGIN
  require(ctx && ctx->has_device && a && b && inout && n > 0 && op >= 0 && op <= 4, -1, "!!ERROR!! mcgpu_kat_f32: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  const size_t nb = (size_t)n * 4;
  float* d = dev.alloc<float>(3 * nb);
  HIP_TRY(hipMemcpy(d, a, nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + n, b, nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + 2 * (size_t)n, inout, nb, hipMemcpyHostToDevice));
  HIP_TRY(launch_kat_f32(op, n, d, d + n, d + 2 * (size_t)n, nullptr));
  HIP_TRY(hipMemcpy(inout, d + 2 * (size_t)n, nb, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_expf(mcgpu_ctx* ctx, int n, const float* x, float* out_exp) {
  ABI_BEGIN
  require(ctx && ctx->has_device && x && out_exp && n > 0, -1, "!!ERROR!! mcgpu_kat_expf: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  const size_t nb = (size_t)n * 4;
  float* d = dev.alloc<float>(2 * nb);
  HIP_TRY(hipMemcpy(d, x, nb, hipMemcpyHostToDevice));
  HIP_TRY(launch_kat_expf(n, d, d + n, nullptr));
  HIP_TRY(hipMemcpy(out_exp, d + n, nb, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_kat_tile_records(int n_tiles, const short* indices, uint32_t* out_u32) {
  ABI_BEGIN
  require(n_tiles > 0 && indices && out_u32, -1, "!!ERROR!! mcgpu_kat_tile_records: bad argument");
  for (int t = 0; t < n_tiles; ++t) {
    const TileRecord r = encode_tile_record(indices + (size_t)t * 64);
    out_u32[4 * t + 0] = r.ab;
    out_u32[4 * t + 1] = r.code;
    out_u32[4 * t + 2] = (uint32_t)r.mask;
    out_u32[4 * t + 3] = (uint32_t)(r.mask >> 32);
  }
  return 0;
  ABI_END
}

}  // extern "C"
