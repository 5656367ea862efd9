// model_device.cpp -- the device-resident model of a context: tables, volume, brick grids, LDS layout.
// Replaces init_CUDA_device (docker/mcgpu/MC-GPU_v1.3.cu:2454-2724).
#include "engine_internal.hpp"

namespace mcgpu {

// Majorant mean free path per coarse energy bin (device_model.hpp: LdsLayout::wood): the table is piecewise linear, mfp(E) =
// x_i + E y_i on table bin i, so its minimum over a coarse bin is taken at the ends of its table bins.  One part in 1e6 below that,
// so that the float product the kernel forms (mfp x density x sigma) stays a probability.
std::vector<float> coarse_woodcock(const HostModel& H) {
  const int nv = H.mat.num_values, nc = (nv + (1 << kWoodShift) - 1) >> kWoodShift;
  const double e0 = (double)H.mat.e0, de = 1.0 / (double)H.mat.ide;
  std::vector<float> out((size_t)nc, 0.f);
  for (int c = 0; c < nc; ++c) {
    double lo = 1.0e30;
    for (int i = c << kWoodShift; i < std::min(nv, (c + 1) << kWoodShift); ++i) {
      const double x = (double)H.mat.woodcock[i].x, y = (double)H.mat.woodcock[i].y;
      lo = std::min(lo, std::min(x + (e0 + i * de) * y, x + (e0 + (i + 1) * de) * y));
    }
    out[(size_t)c] = (float)(lo * (1.0 - 1.0e-6));
  }
  return out;
}

// The object region of a u8 volume and the bricks outside it.  `object[b]` != 0: brick b holds something that is not homogeneous
// background.  Region = the bounding box of those bricks AND -- bodies in a CBCT volume are round, a quarter of their bounding box
// is corner air -- an elliptic cylinder (axis z) with the centre and the aspect of that box, scaled until every corner of every
// object brick is inside; kept only if it puts at least 5 % of the box's bricks outside (else the kernel would pay its quadratic
// for nothing; MCGPU_NO_ELLIPSE: never).  Sets D.objbox_*, D.ell_*, D.has_exterior, D.bricks_exterior; exterior[b] != 0: brick b lies
// wholly outside the region.  Shared by the upload of a geometry and by the device-side geometry change (brick_codes).
static void mark_exterior_region(const HostModel& H, DeviceModel& D, const std::vector<unsigned char>& object, bool have_background,
                                 std::vector<unsigned char>& exterior) {
  const int k = D.brick_shift, nvx[3] = {H.voxels.n[0], H.voxels.n[1], H.voxels.n[2]};
  exterior.assign((size_t)D.brick_count, 0);
  D.has_exterior = 0;
  D.bricks_exterior = 0;
  D.ell_inv[0] = D.ell_inv[1] = 0.f;
  int lo[3] = {D.brick_n[0], D.brick_n[1], D.brick_n[2]}, hi[3] = {-1, -1, -1};
  auto coords = [&](int b, int c3[3]) { c3[0] = b % D.brick_n[0]; c3[1] = (b / D.brick_n[0]) % D.brick_n[1]; c3[2] = b / (D.brick_n[0] * D.brick_n[1]); };
  for (int b = 0; b < D.brick_count; ++b) {
    if (!object[(size_t)b]) continue;
    int c3[3];
    coords(b, c3);
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c3[a]); hi[a] = std::max(hi[a], c3[a]); }
  }
  if (!have_background || hi[0] < 0 || D.knobs.no_exterior) return;
  const float bs = (float)(1 << k);
  auto brick_rect = [&](const int c3[3], float r[4]) {
    r[0] = (float)c3[0] * bs * H.voxels.voxel_size[0]; r[1] = std::min((float)(c3[0] + 1) * bs, (float)nvx[0]) * H.voxels.voxel_size[0];
    r[2] = (float)c3[1] * bs * H.voxels.voxel_size[1]; r[3] = std::min((float)(c3[1] + 1) * bs, (float)nvx[1]) * H.voxels.voxel_size[1];
  };
  float box_lo[3], box_hi[3];
  for (int a = 0; a < 3; ++a) {
    box_lo[a] = (float)(lo[a] << k) * H.voxels.voxel_size[a];
    box_hi[a] = (float)std::min((hi[a] + 1) << k, nvx[a]) * H.voxels.voxel_size[a];
  }
  const float ecx = 0.5f * (box_lo[0] + box_hi[0]), ecy = 0.5f * (box_lo[1] + box_hi[1]);
  const float ea = 0.5f * (box_hi[0] - box_lo[0]), eb = 0.5f * (box_hi[1] - box_lo[1]);
  float inv[2] = {0.f, 0.f};
  if (ea > 0.f && eb > 0.f && !knob_set("MCGPU_NO_ELLIPSE")) {
    double s2 = 0.0;
    for (int b = 0; b < D.brick_count; ++b) {
      if (!object[(size_t)b]) continue;
      int c3[3];
      float r[4];
      coords(b, c3);
      brick_rect(c3, r);
      for (int c = 0; c < 4; ++c) {
        const double dx = ((c & 1) ? r[1] : r[0]) - ecx, dy = ((c & 2) ? r[3] : r[2]) - ecy;
        s2 = std::max(s2, dx * dx / ((double)ea * ea) + dy * dy / ((double)eb * eb));
      }
    }
    s2 *= 1.0 + 1.0e-4;
    inv[0] = (float)(1.0 / (s2 * (double)ea * ea));
    inv[1] = (float)(1.0 / (s2 * (double)eb * eb));
  }
  auto outside_cylinder = [&](const int c3[3]) {  // wholly outside: the point of the brick's rectangle nearest to the axis is
    float r[4];
    brick_rect(c3, r);
    const float px = std::min(std::max(ecx, r[0]), r[1]) - ecx, py = std::min(std::max(ecy, r[2]), r[3]) - ecy;
    return px * px * inv[0] + py * py * inv[1] > 1.001f;
  };
  long in_box = 0, cut = 0;
  if (inv[0] > 0.f) {
    for (int b = 0; b < D.brick_count; ++b) {
      int c3[3];
      coords(b, c3);
      if (c3[0] < lo[0] || c3[0] > hi[0] || c3[1] < lo[1] || c3[1] > hi[1] || c3[2] < lo[2] || c3[2] > hi[2]) continue;
      ++in_box;
      cut += outside_cylinder(c3) ? 1 : 0;
    }
    if (cut * 20 < in_box) inv[0] = inv[1] = 0.f;  // the cylinder would hardly trim the box: not worth its arithmetic
  }
  long outside = 0;
  for (int b = 0; b < D.brick_count; ++b) {
    int c3[3];
    coords(b, c3);
    bool out = c3[0] < lo[0] || c3[0] > hi[0] || c3[1] < lo[1] || c3[1] > hi[1] || c3[2] < lo[2] || c3[2] > hi[2];
    if (!out && inv[0] > 0.f) out = outside_cylinder(c3);
    if (out) { exterior[(size_t)b] = 1; ++outside; }
  }
  if (outside == 0) return;
  D.has_exterior = 1;
  D.bricks_exterior = (int)outside;
  for (int a = 0; a < 3; ++a) { D.objbox_lo[a] = box_lo[a]; D.objbox_hi[a] = box_hi[a]; }
  D.ell_c[0] = ecx; D.ell_c[1] = ecy;
  D.ell_inv[0] = inv[0]; D.ell_inv[1] = inv[1];
}

void read_env_knobs(DeviceModel& D) {
  auto env_int = [](const char* name, int dflt) { return knob_int(name, dflt); };
  DeviceModel::Knobs k;
  k.exterior_mode = env_int("MCGPU_EXTERIOR_MODE", 3);
  k.compat_thresh[0] = env_int("MCGPU_COMPAT_THRESH_COMPTON", -1);
  k.compat_thresh[1] = env_int("MCGPU_COMPAT_THRESH_RAYLEIGH", -1);
  k.compat_thresh[2] = env_int("MCGPU_COMPAT_THRESH_NEW", -1);
  k.compat_thresh[3] = env_int("MCGPU_COMPAT_THRESH_TAKE", -1);
  k.compat_stats = env_int("MCGPU_COMPAT_STATS", 0) != 0;
  k.blocks_per_cu = std::max(0, env_int("MCGPU_BLOCKS_PER_CU", 0));
  k.grid_spare_percent = std::max(0, env_int("MCGPU_GRID_SPARE_PERCENT", 0));
  static const char* const kSched[5] = {"MCGPU_THRESH_COMPTON", "MCGPU_THRESH_RAYLEIGH", "MCGPU_THRESH_NEW", "MCGPU_FLYABLE_LOW", "MCGPU_SWAP_BATCH"};
  for (int i = 0; i < 5; ++i) k.sched_override[i] = env_int(kSched[i], -1);
  k.slot_trade = env_int("MCGPU_SLOT_TRADE", 3);
  k.hold_q = env_int("MCGPU_HOLD_Q", 6) & 15;
  k.no_exterior = knob_set("MCGPU_NO_EXTERIOR");
  k.fast_sched = env_int("MCGPU_FAST_SCHED", D.knobs.fast_sched) != 0 ? 1 : 0;
  k.segment_loop = env_int("MCGPU_SEGMENT_LOOP", -1);
  k.tally_stage = env_int("MCGPU_TALLY_STAGE", -1);
  k.tally_stage = k.tally_stage < 0 ? -1 : (k.tally_stage != 0 ? 1 : 0);
  k.stage_cap = std::max(0, env_int("MCGPU_TALLY_STAGE_CAP", 0));
  k.stage_max_histories = (unsigned long long)std::max(1, env_int("MCGPU_TALLY_STAGE_MAX_HISTORIES", 1 << 27));
  D.knobs = k;
}

// The FAST scheduler's parameters live in TrackCold (device memory read through the scalar cache): effective value =
// environment override, else the schedule set by mcgpu_set_fast_schedule.  Uploads only when something changed, after the
// device has drained (callers are set-up paths, never a launch).
void apply_schedule(DeviceModel& D) {
  if (!D.cold) return;
  TrackCold& ch = D.cold_host;
  int want[5];
  // the workgroup-level pool fills its batches from the whole workgroup: its thresholds are "lanes a batch must fill"
  static const int kWgSched[5] = {56, 56, 56, 40, 40};
  for (int i = 0; i < 5; ++i)
    want[i] = D.knobs.sched_override[i] >= 0 ? D.knobs.sched_override[i] : ((D.knobs.fast_sched == 1 && !D.sched_set) ? kWgSched[i] : D.sched[i]);
  want[3] = std::max(1, want[3]);
  want[4] = std::max(1, want[4]);
  // bit 0: slots traded before flight, bit 1: before the Compton and tally/source services; bits 8-11: hold_q (sixteenths
  // of the flying lanes that end a flight segment at the latest)
  const int trade = D.knobs.slot_trade | (D.knobs.hold_q << 8);
  if (ch.trade_slots == trade && ch.thresh_compton == want[0] && ch.thresh_rayleigh == want[1] && ch.thresh_new == want[2] && ch.flyable_low == want[3] &&
      ch.swap_batch == want[4])
    return;
  ch.thresh_compton = want[0]; ch.thresh_rayleigh = want[1]; ch.thresh_new = want[2]; ch.flyable_low = want[3]; ch.swap_batch = want[4];
  ch.trade_slots = trade;
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(D.cold, &ch, sizeof ch, hipMemcpyHostToDevice));
}

// COMPAT kernel: bounds of S0(E) = sum_i f_i n_i(E, theta = pi) (K.cu:1300-1314), the normalisation of the Compton angle test
// "xi S0 > S(theta) T(tau)" (K.cu:1367-1372).  Computing it costs a second pass over the 29-40 electron shells of a tissue per
// event -- 46 % of the kernel's Compton work -- and the test rarely needs its exact value.  S0 does not decrease with E: a
// shell enters at E > U_i with a positive term, and each term grows with E (p_z(theta = pi) grows with E (E - U_i), the
// profile integral n_i with p_z).  So S0 at the lower / upper edge of an energy bin bounds it inside the bin.  The edges are
// evaluated here in double, one bin of slack on either side absorbs the float rounding of the kernel's bin index, and a
// relative margin of 1e-4 covers the float arithmetic of the reference's own S0 (terms accurate to ~2e-6 of f_i, forty
// additions of 6e-8 each).  A test that both bounds decide alike is decided; for the rest (well below 1 % with 1024 bins) the kernel computes S0.
// Layout: float2 {lo, hi} at [row * kS0Bins + bin]; row = compact material index with `compact_of`, else material number - 1.
static std::vector<float> build_s0_bounds(const HostModel& H, const int* compact_of, int rows, float* emin_out, float* inv_w_out) {
  const double emin = H.mat.e0, emax = H.mat.e0 + (double)(H.mat.num_values - 1) / H.mat.ide, w = (emax - emin) / kS0Bins;
  const double mc2 = (double)510998.918f, c1 = (double)0.707106781186545f, c2 = (double)1.4142135623731f;
  std::vector<float> bounds((size_t)2 * kS0Bins * std::max(rows, 1), 0.f);
  for (int m = 0; m < kMaxMaterials; ++m) {
    const int mc = compact_of ? compact_of[m] : (m < rows ? m : -1);
    if (mc < 0) continue;
    const int n = std::min(H.mat.noscco[m], kMaxShells);
    double fsum = 0.0;
    for (int i = 0; i < n; ++i) fsum += (double)H.mat.fco[m + i * kMaxMaterials];
    auto s0_at = [&](double E) {
      double acc = 0.0;
      for (int i = 0; i < n; ++i) {
        const double U = H.mat.uico[m + i * kMaxMaterials], J = H.mat.fj0[m + i * kMaxMaterials], f = H.mat.fco[m + i * kMaxMaterials];
        if (!(U < E)) continue;
        const double aux = E * (E - U) * 2.0;
        const double pz = J * (aux - U * mc2) / (std::sqrt(aux + aux + U * U) * mc2);
        const double a = pz > 0.0 ? c1 + pz * c2 : c1 - pz * c2;
        const double t = 0.5 * std::exp(0.5 - a * a);
        acc += f * (pz > 0.0 ? 1.0 - t : t);
      }
      return acc;
    };
    // the monotonicity argument needs shells with f >= 0, J > 0, U >= 0 (every PENELOPE table has them); a file that breaks it
    // gets bounds that decide nothing: the kernel then computes S0 for every test, like the reference
    bool regular = true;
    for (int i = 0; i < n; ++i)
      regular = regular && H.mat.fco[m + i * kMaxMaterials] >= 0.f && H.mat.fj0[m + i * kMaxMaterials] > 0.f && H.mat.uico[m + i * kMaxMaterials] >= 0.f;
    if (!regular) {
      for (int k = 0; k < kS0Bins; ++k) {
        bounds[2 * ((size_t)mc * kS0Bins + k)] = 0.f;
        bounds[2 * ((size_t)mc * kS0Bins + k) + 1] = 3.0e38f;
      }
      continue;
    }
    std::vector<double> edge(kS0Bins + 1);
    for (int k = 0; k <= kS0Bins; ++k) edge[k] = s0_at(emin + k * w);
    for (int k = 0; k < kS0Bins; ++k) {
      const double lo = k >= 1 ? edge[k - 1] * (1.0 - 1e-4) : 0.0;
      const double hi = (k + 2 <= kS0Bins ? edge[k + 2] : fsum) * (1.0 + 1e-4);
      bounds[2 * ((size_t)mc * kS0Bins + k)] = std::nextafterf((float)lo, -1.0f);
      bounds[2 * ((size_t)mc * kS0Bins + k) + 1] = std::nextafterf((float)hi, 3.0e38f);
    }
  }
  if (emin_out) *emin_out = (float)emin;
  if (inv_w_out) *inv_w_out = (float)(1.0 / w);
  return bounds;
}

// ---- device memory of a model
void DeviceOwner::claim() {
  if (device_ < 0) HIP_TRY(hipGetDevice(&device_));
}
void* DeviceOwner::device_bytes(size_t bytes) {
  claim();
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  buffers_.push_back(p);
  return p;
}
void* DeviceOwner::pinned_bytes(size_t bytes, unsigned int flags) {
  claim();
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, bytes, flags));
  pinned_.push_back(p);
  return p;
}
hipStream_t DeviceOwner::stream(unsigned int flags) {
  claim();
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, flags));
  streams_.push_back(s);
  return s;
}
hipEvent_t DeviceOwner::event(unsigned int flags) {
  claim();
  hipEvent_t e = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&e, flags));
  events_.push_back(e);
  return e;
}
void DeviceOwner::free(void* device_buffer) {
  auto it = std::find(buffers_.begin(), buffers_.end(), device_buffer);
  if (it == buffers_.end()) return;
  buffers_.erase(it);
  HIP_TRY(hipFree(device_buffer));
}
void DeviceOwner::swap(DeviceOwner& o) noexcept {
  std::swap(device_, o.device_);
  buffers_.swap(o.buffers_);
  pinned_.swap(o.pinned_);
  streams_.swap(o.streams_);
  events_.swap(o.events_);
}
DeviceOwner::~DeviceOwner() {
  if (device_ < 0) return;
  int current = -1;
  const bool restore = hipGetDevice(&current) == hipSuccess && current != device_;
  (void)hipSetDevice(device_);
  for (void* p : buffers_) (void)hipFree(p);
  for (void* p : pinned_) (void)hipHostFree(p);
  for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
  for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  if (restore) (void)hipSetDevice(current);
}

// ---- stages of upload_model
static void select_device(DeviceModel& D, int device_id) {
  HIP_TRY(hipSetDevice(device_id));
  D.device_id = device_id;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  D.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  read_env_knobs(D);
}

static int compact_numbering(const HostModel& H, int compact_of[kMaxMaterials]) {
  int n = 0;
  for (int m = 0; m < kMaxMaterials; ++m) compact_of[m] = H.mat.used[m] ? n++ : -1;
  return n;
}

static int total_shells(const HostModel& H, const int* compact_of) {
  int shells = 0;
  for (int m = 0; m < kMaxMaterials; ++m)
    if (compact_of[m] >= 0) shells += std::min(H.mat.noscco[m], kMaxShells);
  return shells;
}

// One entry {density, bits(compact material)} per distinct (material, density) pair of the volume, and each voxel's entry.
struct Palette {
  std::vector<float> entries;
  std::vector<uint16_t> index;  // incomplete when `overflow`
  bool overflow = false;        // more than 65536 pairs: the volume is stored raw
  int size() const { return (int)(entries.size() / 2); }
};

static Palette build_palette(const HostModel& H, const int* compact_of) {
  const size_t nvox = H.voxels.count();
  Palette P;
  P.index.resize(nvox);
  std::unordered_map<uint64_t, int> index_of;
  auto key_of = [](int material, float density) { uint32_t db; memcpy(&db, &density, 4); return ((uint64_t)material << 32) | db; };
  auto add = [&](uint64_t key, float density, int mc) {
    float mcf;
    memcpy(&mcf, &mc, 4);
    const int at = (int)index_of.size();
    index_of.emplace(key, at);
    P.entries.push_back(density);
    P.entries.push_back(mcf);
    return at;
  };
  uint64_t last_key = ~0ull;
  int last_idx = -1;
  for (size_t i = 0; i < nvox; ++i) {
    const uint64_t key = key_of(H.voxels.material[i], H.voxels.density[i]);
    if (key != last_key) {
      auto it = index_of.find(key);
      if (it != index_of.end()) {
        last_idx = it->second;
      } else {
        if (index_of.size() >= 65536) { P.overflow = true; return P; }
        const int mc = compact_of[H.voxels.material[i] - 1];
        if (mc < 0) throw Error(-2, "!!ERROR!! A voxel uses material " + std::to_string((int)H.voxels.material[i]) + " but no data file was given for it.");
        last_idx = add(key, H.voxels.density[i], mc);
      }
      last_key = key;
    }
    P.index[i] = (uint16_t)last_idx;
  }
  // the reference's default for voxels warped in from outside the volume (air: material 1 at 0.0013 g/cm^3,
  // cbctmc/mc/geometry.py:403-418) gets an entry of a u8 palette even when no voxel holds it yet, so that a geometry can be
  // warped on the device without touching the palette (mcgpu_warp_geometry)
  const uint64_t air = key_of(1, 0.0013f);
  if (P.size() < 256 && compact_of[0] >= 0 && !index_of.count(air)) add(air, 0.0013f, compact_of[0]);
  return P;
}

static std::vector<float> raw_volume(const HostModel& H, const int* compact_of) {
  const size_t nvox = H.voxels.count();
  std::vector<float> raw(2 * nvox);
  for (size_t i = 0; i < nvox; ++i) {
    const int mc = compact_of[H.voxels.material[i] - 1];
    if (mc < 0) throw Error(-2, "!!ERROR!! A voxel uses a material without data file.");
    raw[2 * i] = H.voxels.density[i];
    memcpy(&raw[2 * i + 1], &mc, 4);
  }
  return raw;
}

// Device layout of a u8 volume: tiles of 4x4x4 voxels = one 64-byte sector = one sub-brick of the second level (device_model.hpp:
// tiled_voxel); the padding voxels of edge tiles repeat the tile's first voxel and are never addressed.
static std::vector<uint8_t> tiled_volume(const VoxelGrid& V, const std::vector<uint8_t>& idx8) {
  const int nx = V.n[0], ny = V.n[1], nz = V.n[2];
  const unsigned int snx = (unsigned int)((nx + 3) >> 2), sny = (unsigned int)((ny + 3) >> 2), snz = (unsigned int)((nz + 3) >> 2);
  const size_t tiles = (size_t)snx * sny * snz;
  if (tiles * 64 >= (1ULL << 31)) throw Error(-2, "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  std::vector<uint8_t> tiled(tiles * 64);
  for (size_t t = 0; t < tiles; ++t) {
    const int x0 = (int)(t % snx) << 2, y0 = (int)((t / snx) % sny) << 2, z0 = (int)(t / ((size_t)snx * sny)) << 2;
    const uint8_t pad = idx8[((size_t)z0 * ny + y0) * nx + x0];
    for (int dz = 0; dz < 4; ++dz)
      for (int dy = 0; dy < 4; ++dy)
        for (int dx = 0; dx < 4; ++dx) {
          const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
          tiled[t * 64 + (size_t)(dz * 16 + dy * 4 + dx)] = (x < nx && y < ny && z < nz) ? idx8[((size_t)z * ny + y) * nx + x] : pad;
        }
  }
  return tiled;
}

// ---- LDS image of the kernels (byte offsets; track_common.inc: stage_tables): its regions in order, each on 16 bytes, closed by
// the FAST kernel's cross-section brackets at their shift.  One description for the brick-grid budget and for the layout.
constexpr int kLdsPerWorkgroup = 160 * 1024 / 2;  // two 1024-thread workgroups per CU
// The budget that picks brick_shift bounds the image instead of laying it out: every region start and the end may round up by
// 16 bytes -- 13 such boundaries counted in full -- so that the choice never depends on the padding between the regions.
constexpr int kLdsAlignSlack = 13 * 16;

struct LdsPlan {
  struct Region {
    int LdsLayout::*at;
    int bytes;
  };
  std::vector<Region> regions;  // the brackets excluded
  int nv = 0, nmat = 0;
};

static int coarse_bins(int nv, int shift) { return (nv + (1 << shift) - 1) >> shift; }

static LdsPlan plan_lds(const HostModel& H, const DeviceModel& D, int brick_bytes) {
  const int ns = std::min(H.spectrum.num_bins + 1, kMaxSpectrumBins) + 1;
  const bool u8 = D.vol_kind == kVolU8;
  LdsPlan P;
  P.nv = H.mat.num_values;
  P.nmat = D.nmat;
  P.regions = {{&LdsLayout::shells, std::max(total_shells(H, D.compact_of), 1) * 16},
               {&LdsLayout::nosc, std::max(D.nmat, 1) * 8},
               {&LdsLayout::espc, ns * 4},
               {&LdsLayout::cutoff, ns * 4},
               {&LdsLayout::alias, ns * 2},
               {&LdsLayout::pal, u8 ? (16 + D.palette_size) * 8 : 0},
               {&LdsLayout::brick, u8 ? brick_bytes : 0},
               {&LdsLayout::dose_mat, 2 * kMaxMaterials * 8},
               {&LdsLayout::slots, kSlotWords * kPoolParked * kPoolBlockThreads * 4}};  // the COMPAT kernel's image ends at `slots`
  if (D.knobs.fast_sched == 1) P.regions.push_back({&LdsLayout::queues, kPoolQueueBytes});
  P.regions.push_back({&LdsLayout::wood, coarse_bins(P.nv, kWoodShift) * 4});
  return P;
}

// sig_shift < 0: no brackets
static LdsLayout lay_out_lds(const LdsPlan& P, int sig_shift) {
  LdsLayout Y{};
  int off = 0;
  auto take = [&](int bytes) { off = (off + 15) / 16 * 16; const int at = off; off += bytes; return at; };
  for (const LdsPlan::Region& r : P.regions) Y.*r.at = take(r.bytes);
  Y.sig_mid = Y.sig_w = off;
  if (sig_shift >= 0) {
    const int nc = coarse_bins(P.nv, sig_shift);
    Y.sig_mid = take(nc * P.nmat * 2);
    Y.sig_w = take(nc * 4);
  }
  Y.total = (off + 15) / 16 * 16;
  return Y;
}

// Bound of the image without its brick grid, with brackets no coarser than 2^9 table bins.
static long lds_bytes_without_bricks(const LdsPlan& P) {
  const int nc = coarse_bins(P.nv, 9);
  long bytes = kLdsAlignSlack + (long)nc * P.nmat * 2 + nc * 4;
  for (const LdsPlan::Region& r : P.regions) bytes += r.bytes;
  return bytes;
}

// Brick grid: the smallest power-of-two brick (>= 4 voxels) that keeps the grid within the LDS budget.  The FAST kernel wants two
// 1024-thread workgroups per CU, i.e. an LDS image of at most 80 KB.  Everything but the brick grid is fixed by the materials in
// use (22 tissue materials: 458 Compton shells = 7.3 KB against 1.4 KB for the Catphan set), so the grid gets what is left after
// the tables, the history slots and a coarse bracket table.
static int choose_brick_shift(const HostModel& H, const DeviceModel& D) {
  auto nb = [](int n, int sh) { return (n + (1 << sh) - 1) >> sh; };
  const char* mb = knob_str("MCGPU_MAX_BRICKS");  // tuning knob: a coarser grid frees LDS
  long max_bricks = mb ? std::min<long>(std::max<long>(atol(mb), 1), kMaxBricks) : kMaxBricks;
  const long left = kLdsPerWorkgroup - lds_bytes_without_bricks(plan_lds(H, D, 0));
  if (left > 0) max_bricks = std::min(max_bricks, std::max(2 * left, 512L));
  int k = 2;
  while ((long)nb(H.voxels.n[0], k) * nb(H.voxels.n[1], k) * nb(H.voxels.n[2], k) > max_bricks) ++k;
  return k;
}

// Per brick and per sub-brick of 4^3 voxels: the palette entry of a homogeneous one, kMixedBrick for one that holds more.  One pass
// over the voxels (134 M at 512^3).
struct BrickClasses {
  std::vector<unsigned short> brick, sub;
};

static BrickClasses classify_bricks(const HostModel& H, const DeviceModel& D, const std::vector<uint8_t>& idx8) {
  const int nx = H.voxels.n[0], ny = H.voxels.n[1], nz = H.voxels.n[2], k = D.brick_shift;
  BrickClasses c;
  c.brick.assign((size_t)D.brick_count, 0xFFFF);
  c.sub.assign((size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2], 0xFFFF);
  auto see = [](unsigned short& f, int v) {
    if (f == 0xFFFF) f = (unsigned short)v;
    else if (f != v) f = kMixedBrick;
  };
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y) {
      const size_t row = ((size_t)z * ny + y) * nx;
      unsigned short* brow = &c.brick[((size_t)(z >> k) * D.brick_n[1] + (y >> k)) * D.brick_n[0]];
      unsigned short* srow = &c.sub[((size_t)(z >> 2) * D.sub_n[1] + (y >> 2)) * D.sub_n[0]];
      for (int x = 0; x < nx; ++x) {
        const int v = idx8[row + x];
        see(brow[x >> k], v);
        see(srow[x >> 2], v);
      }
    }
  return c;
}

// 4-bit codes: the 14 most frequent palette entries among homogeneous bricks get codes 0..13, every other brick (mixed, or a rarer
// homogeneous one) is 0xF = "read the voxel"; code 14 = EXTERIOR (brick_codes).  Returns whether any brick is homogeneous background.
static bool assign_codes(DeviceModel& D, const std::vector<unsigned short>& brick_first) {
  std::vector<long> homogeneous(256, 0);
  for (unsigned short f : brick_first)
    if (f < kMixedBrick) ++homogeneous[f];
  std::vector<int> order(256);
  for (int i = 0; i < 256; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return homogeneous[a] > homogeneous[b]; });
  for (int i = 0; i < 256; ++i) D.code_of[i] = 0xF;
  for (int c = 0; c < 16; ++c) D.brick_palette[c] = 0;
  for (int c = 0; c < 14; ++c)
    if (homogeneous[order[c]] > 0) { D.code_of[order[c]] = (unsigned char)c; D.brick_palette[c] = order[c]; }
  D.background = order[0];
  return homogeneous[order[0]] > 0;
}

// 4-bit code tables (bricks, sub-bricks): code i in the low nibble of byte i / 2 for even i, in the high one for odd i; a spare
// nibble is 0xF.
static std::vector<unsigned char> pack_codes(const std::vector<unsigned char>& codes) {
  std::vector<unsigned char> packed((codes.size() + 1) / 2, 0xFF);
  for (size_t i = 0; i < codes.size(); ++i) {
    const int sh = (int)(i & 1) * 4;
    packed[i >> 1] = (unsigned char)((packed[i >> 1] & ~(0xF << sh)) | (codes[i] << sh));
  }
  return packed;
}

// Exterior (mark_exterior_region): outside the object region every brick is homogeneous background, and the FAST kernel crosses
// it with one exact free-path sample instead of delta-tracking through it (track_pool.inc: exterior_hop).  Sets the region,
// D.bricks_mixed and D.bricks_exterior.
std::vector<unsigned char> brick_codes(const HostModel& H, DeviceModel& D, const std::vector<unsigned short>& brick_first,
                                       bool have_background) {
  std::vector<unsigned char> object((size_t)D.brick_count), exterior;
  for (int b = 0; b < D.brick_count; ++b) object[(size_t)b] = brick_first[(size_t)b] != D.background ? 1 : 0;
  mark_exterior_region(H, D, object, have_background, exterior);
  std::vector<unsigned char> codes((size_t)D.brick_count);
  D.bricks_mixed = 0;
  for (int b = 0; b < D.brick_count; ++b) {
    const unsigned short f = brick_first[(size_t)b];
    codes[(size_t)b] = exterior[(size_t)b] ? 14 : (f == kMixedBrick ? 0xF : D.code_of[f]);
    D.bricks_mixed += (codes[(size_t)b] == 0xF);
  }
  // code 14 means "background outside the object region": its palette slot must name the background even when the BASE
  // geometry of a warp had no exterior (its object box spanned the whole brick grid) and the warp made one
  if (D.has_exterior) D.brick_palette[14] = D.background;
  return pack_codes(codes);
}

static void upload_sub_bricks(DeviceModel& D, const std::vector<unsigned short>& sub_first) {
  // Second-level codes (same 4-bit coding, no EXTERIOR): a flight step that lands in a mixed brick asks this table,
  // which stays in L2 (0.5-1 MB), before it asks the volume (64-128 MiB: Infinity Cache / HBM).  On a body-filling
  // volume 78 % of the tissue voxels lie in mixed 16^3 bricks but only 24 % in mixed 4^3 sub-bricks, and the voxel
  // gathers of the flight step were what bound that workload (1.45 KB of fabric traffic per history at 5e9 histories/s).
  // Round 2 (x-fastest rows): worth its dependent L2 round trip where most bricks a photon meets are mixed (thorax +24 %).
  // Round 3: the volume is stored in 4x4x4 TILES, one tile = one 64-byte sector = one sub-brick -- asking the volume
  // directly now costs one sector like asking this table, without the second dependent round trip, and the tile it
  // brings in serves the neighbouring voxels of later photons.  Measured on one box (tools/ab_second_level.sh): thorax 14.27
  // -> 13.68 ms, CIRS 6.52 -> 6.25, Catphan 4.17 -> 4.09 with the table OFF.  So it is off unless MCGPU_SUB_BRICKS=1
  // asks for it (kept: it halves the fabric traffic where that is what binds, and the tests hold both routes to the
  // same tallies).
  const char* knob = knob_str("MCGPU_SUB_BRICKS");
  const bool on = knob && atoi(knob) != 0;
  std::vector<unsigned char> codes(sub_first.size());
  D.sub_mixed = 0;
  for (size_t b = 0; b < sub_first.size(); ++b) {
    codes[b] = (on && sub_first[b] < kMixedBrick) ? D.code_of[sub_first[b]] : 0xF;
    D.sub_mixed += (codes[b] == 0xF);
  }
  D.sub = on ? D.put(pack_codes(codes)) : nullptr;
}

// Whether this model keeps tile records (the comment in upload_tile_records says when they pay); sets D.tiles_in_mixed_bricks and D.rec_n.
static bool want_tile_records(DeviceModel& D, const std::vector<unsigned short>& brick_first) {
  const int k = D.brick_shift;
  const size_t nsub = (size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2];
  long long hot_tiles = 0;
  for (size_t b = 0; b < nsub; ++b) {
    const int bx = (int)((b % D.sub_n[0]) << 2) >> k, by = (int)(((b / D.sub_n[0]) % D.sub_n[1]) << 2) >> k, bz = (int)((b / ((size_t)D.sub_n[0] * D.sub_n[1])) << 2) >> k;
    hot_tiles += brick_first[((size_t)bz * D.brick_n[1] + by) * D.brick_n[0] + bx] == kMixedBrick ? 1 : 0;
  }
  D.tiles_in_mixed_bricks = hot_tiles;
  D.rec_n[0] = (D.sub_n[0] + 1) >> 1; D.rec_n[1] = (D.sub_n[1] + 1) >> 1; D.rec_n[2] = (D.sub_n[2] + 1) >> 1;
  const char* knob = knob_str("MCGPU_TILE_RECORDS");
  return knob ? atoi(knob) != 0 : hot_tiles * 64 > (8LL << 20);
}

static void upload_tile_records(const HostModel& H, DeviceModel& D, const std::vector<uint8_t>& idx8, const std::vector<unsigned short>& brick_first) {
  // Tile records (device_model.hpp: TileRecord): the hot set of the voxel gathers is every 64-byte tile of every MIXED brick.
  // Where that set is far beyond the L2 (4 MB per XCD) -- body-filling tissue volumes: thorax 22 MB -- the launch is bound by
  // the line fills of those gathers (profiles/r04p_*: ONE more cold line per mixed step doubles the thorax's kernel time, one
  // more load from the SAME line costs 2 %), and the records shrink the set fourfold.  MCGPU_TILE_RECORDS=0/1 overrides.
  const int nx = H.voxels.n[0], ny = H.voxels.n[1], nz = H.voxels.n[2];
  const size_t nsub = (size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2];
  D.tile_rec = nullptr;
  if (!want_tile_records(D, brick_first)) return;
  std::vector<TileRecord> rec((size_t)D.rec_n[0] * D.rec_n[1] * D.rec_n[2] * 8, TileRecord{0u, 0u, 0ULL});
  for (size_t t = 0; t < nsub; ++t) {
    const unsigned int tx = (unsigned int)(t % D.sub_n[0]), ty = (unsigned int)((t / D.sub_n[0]) % D.sub_n[1]), tz = (unsigned int)(t / ((size_t)D.sub_n[0] * D.sub_n[1]));
    short v64[64];
    for (int v = 0; v < 64; ++v) {
      const int x = (int)(tx << 2) + (v & 3), y = (int)(ty << 2) + ((v >> 2) & 3), z = (int)(tz << 2) + (v >> 4);
      v64[v] = (x >= nx || y >= ny || z >= nz) ? (short)-1 : (short)idx8[((size_t)z * ny + y) * nx + x];  // padding of an edge tile: never addressed
    }
    rec[tile_record_index(tx, ty, tz, (unsigned int)D.rec_n[0], (unsigned int)(D.rec_n[0] * D.rec_n[1]))] = encode_tile_record(v64);
  }
  D.tile_rec = D.put(rec);
}

// u8 volumes: brick grid, first- and second-level codes, tile records
static void size_brick_grids(const HostModel& H, DeviceModel& D) {
  const int k = choose_brick_shift(H, D);
  D.brick_shift = k;
  for (int a = 0; a < 3; ++a) {
    D.brick_n[a] = (H.voxels.n[a] + (1 << k) - 1) >> k;
    D.sub_n[a] = (H.voxels.n[a] + 3) >> 2;
  }
  D.brick_count = D.brick_n[0] * D.brick_n[1] * D.brick_n[2];
  D.brick_bytes = (D.brick_count + 1) / 2;
}

static void upload_brick_grids(const HostModel& H, DeviceModel& D, const std::vector<uint8_t>& idx8) {
  size_brick_grids(H, D);
  const BrickClasses c = classify_bricks(H, D, idx8);
  const bool have_background = assign_codes(D, c.brick);
  D.bricks = D.put(brick_codes(H, D, c.brick, have_background));
  upload_sub_bricks(D, c.sub);
  upload_tile_records(H, D, idx8, c.brick);
}

// The palette-compressed volume: u8 (tiled, with brick grids) up to 256 palette entries, u16 up to 65536, else raw.
static void upload_volume(const HostModel& H, DeviceModel& D) {
  const Palette P = build_palette(H, D.compact_of);
  if (P.overflow) {
    const std::vector<float> raw = raw_volume(H, D.compact_of);
    D.vol_kind = kVolRaw;
    D.vol = D.put(raw);
    D.vol_bytes = raw.size() * 4;
    D.palette_size = 0;
    D.palette = D.put(std::vector<float>(2, 0.f));
    return;
  }
  D.palette_size = P.size();
  D.palette = D.put(P.entries);
  if (P.size() > 256) {
    D.vol_kind = kVolU16;
    D.vol = D.put(P.index);
    D.vol_bytes = P.index.size() * 2;
    return;
  }
  D.vol_kind = kVolU8;
  D.palette_host = P.entries;
  const std::vector<uint8_t> idx8(P.index.begin(), P.index.end());
  const std::vector<uint8_t> tiled = tiled_volume(H.voxels, idx8);
  D.vol = D.put(tiled);
  D.vol_bytes = tiled.size();
  upload_brick_grids(H, D, idx8);
}

// The same u8 volume from classes that are already on the device (mcgpu_set_geometry_image; image_map.hip): what upload_volume builds
// from the host arrays of the same geometry, without a voxel-sized pass on the host.
//   palette      : a voxel's (material, density) is its class's, so the first-occurrence order of the [z][y][x] scan (build_palette) is the
//                  order of the classes' smallest voxel index; classes that share a (material, density) pair share an entry; air at
//                  0.0013 is appended when absent, as there.
//   volume       : class -> palette index in one pass (image_map.hip: remap_kernel); the padding of edge tiles was written by the mapping.
//   brick grids  : sub-brick and brick classification and the tile records come from the kernels of the device-side geometry change
//                  (geometry_device.hip; the warp tests hold them to the host's); the code assignment, the object region and the packed
//                  code tables are the host's own functions on the downloaded per-brick results (2 bytes per 64 voxels).
static void upload_volume_from_device(const HostModel& H, DeviceModel& D, const DeviceVolumeSource& src) {
  const size_t tiles = (size_t)((H.voxels.n[0] + 3) >> 2) * ((H.voxels.n[1] + 3) >> 2) * ((H.voxels.n[2] + 3) >> 2);
  if (tiles * 64 >= (1ULL << 31)) throw Error(-2, "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  if (src.bytes != tiles * 64) throw Error(-9, "!!ERROR!! internal: the mapped volume does not have the size of the tiled grid");
  int order[kImageClasses], present = 0;
  for (int c = 0; c < kImageClasses; ++c)
    if (src.first[c] != 0xFFFFFFFFu) order[present++] = c;
  std::sort(order, order + present, [&](int a, int b) { return src.first[a] < src.first[b]; });
  std::vector<float> entries;
  std::vector<uint64_t> keys;
  auto key_of = [](int material, float density) { uint32_t db; memcpy(&db, &density, 4); return ((uint64_t)material << 32) | db; };
  auto add = [&](uint64_t key, float density, int mc) {
    float mcf;
    memcpy(&mcf, &mc, 4);
    keys.push_back(key);
    entries.push_back(density);
    entries.push_back(mcf);
  };
  unsigned char lut[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < present; ++i) {
    const int c = order[i];
    const uint64_t key = key_of(src.material[c], src.density[c]);
    size_t at = std::find(keys.begin(), keys.end(), key) - keys.begin();
    if (at == keys.size()) {
      const int mc = D.compact_of[src.material[c] - 1];
      if (mc < 0) throw Error(-2, "!!ERROR!! A voxel uses material " + std::to_string(src.material[c]) + " but no data file was given for it.");
      add(key, src.density[c], mc);
    }
    lut[c] = (unsigned char)at;
  }
  const uint64_t air = key_of(1, 0.0013f);
  if (D.compact_of[0] >= 0 && std::find(keys.begin(), keys.end(), air) == keys.end()) add(air, 0.0013f, D.compact_of[0]);
  D.palette_size = (int)keys.size();
  D.palette = D.put(entries);
  D.vol_kind = kVolU8;
  D.palette_host = entries;
  D.vol = D.mem.device_bytes(src.bytes);
  D.vol_bytes = src.bytes;
  HIP_TRY(launch_image_remap(src.classes_tiled, (unsigned char*)D.vol, src.bytes, lut, nullptr));
  size_brick_grids(H, D);
  const size_t nsub = (size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2];
  const int rn[3] = {(D.sub_n[0] + 1) >> 1, (D.sub_n[1] + 1) >> 1, (D.sub_n[2] + 1) >> 1};
  const size_t nrec = (size_t)rn[0] * rn[1] * rn[2] * 8;
  unsigned short* sub_first = (unsigned short*)D.mem.device_bytes(nsub * 2);
  unsigned short* brick_first = (unsigned short*)D.mem.device_bytes((size_t)D.brick_count * 2);
  unsigned int* out = (unsigned int*)D.mem.device_bytes(32 * 4);
  TileRecord* rec = (TileRecord*)D.mem.device_bytes(nrec * sizeof(TileRecord));  // kept only where the records pay (want_tile_records)
  HIP_TRY(hipMemsetAsync(rec, 0, nrec * sizeof(TileRecord), nullptr));            // cubes beyond the grid: zero records, as on the host
  GeometryRebuild g{};
  g.nx = H.voxels.n[0]; g.ny = H.voxels.n[1]; g.nz = H.voxels.n[2];
  g.brick_shift = D.brick_shift;
  for (int k = 0; k < 3; ++k) { g.bn[k] = D.brick_n[k]; g.sn[k] = D.sub_n[k]; g.rn[k] = rn[k]; }
  g.idx = (unsigned char*)D.vol;
  g.sub_first = sub_first; g.brick_first = brick_first; g.rec = rec; g.out = out;
  g.background = -1;
  HIP_TRY(launch_geometry_classify(g, nullptr));
  BrickClasses c;
  c.brick.resize((size_t)D.brick_count);
  c.sub.resize(nsub);
  HIP_TRY(hipMemcpy(c.brick.data(), brick_first, c.brick.size() * 2, hipMemcpyDeviceToHost));  // waits for the kernels
  HIP_TRY(hipMemcpy(c.sub.data(), sub_first, c.sub.size() * 2, hipMemcpyDeviceToHost));
  D.mem.free(sub_first);
  D.mem.free(brick_first);
  D.mem.free(out);
  const bool have_background = assign_codes(D, c.brick);
  D.bricks = D.put(brick_codes(H, D, c.brick, have_background));
  upload_sub_bricks(D, c.sub);
  D.tile_rec = nullptr;
  if (want_tile_records(D, c.brick)) D.tile_rec = rec;
  else D.mem.free(rec);
}

// Cross-section records: 8 floats {a, b, pmax, 0} per (compact material, table bin), material-major rows (track_common.inc: table_row)
static std::vector<float> cross_section_records(const HostModel& H, const int* compact_of, int nmat) {
  const int nv = H.mat.num_values;
  std::vector<float> rec(8 * (size_t)nv * nmat, 0.f);
  for (int i = 0; i < nv; ++i)
    for (int m = 0; m < kMaxMaterials; ++m) {
      const int mc = compact_of[m];
      if (mc < 0) continue;
      float* r = &rec[8 * ((size_t)mc * nv + i)];
      const Float3& a = H.mat.a[(size_t)i * kMaxMaterials + m];
      const Float3& b = H.mat.b[(size_t)i * kMaxMaterials + m];
      r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = b.x; r[4] = b.y; r[5] = b.z;
      r[6] = H.mat.pmax[(size_t)(i + 1) * kMaxMaterials + m];
    }
  return rec;
}

// {a_tot, b_tot} of every record
static std::vector<float> total_cross_sections(const std::vector<float>& rec) {
  std::vector<float> tot(rec.size() / 4);
  for (size_t k = 0; k < rec.size() / 8; ++k) { tot[2 * k] = rec[8 * k]; tot[2 * k + 1] = rec[8 * k + 3]; }
  return tot;
}

// The Woodcock table and the FAST kernel's LDS copy of its majorant (coarse_woodcock): allocated at upload, overwritten when a
// geometry change rebuilds the table.
void refresh_woodcock(const HostModel& H, DeviceModel& D) {
  std::vector<float> wood(2 * (size_t)H.mat.num_values);
  for (int i = 0; i < H.mat.num_values; ++i) { wood[2 * i] = H.mat.woodcock[i].x; wood[2 * i + 1] = H.mat.woodcock[i].y; }
  const std::vector<float> coarse = coarse_woodcock(H);
  if (!D.woodcock) {
    D.woodcock = D.put(wood);
    D.wood_coarse = D.put(coarse);
    return;
  }
  HIP_TRY(hipMemcpy(D.woodcock, wood.data(), wood.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.wood_coarse, coarse.data(), coarse.size() * 4, hipMemcpyHostToDevice));
}

// FAST Compton sampler (track_common.inc: compton_draw): Walker alias table of the shell weights f_i of material m (Vose's
// construction, in double): column s keeps shell s below cut[s] and maps the rest of the column to alias[s].  Entries at
// [shell * nmat + mc].
static void shell_alias_table(const HostModel& H, int m, int mc, int nmat, float* cut, unsigned char* alias) {
  const int n = std::min(H.mat.noscco[m], kMaxShells);
  double F = 0.0;
  for (int s = 0; s < n; ++s) F += (double)H.mat.fco[m + s * kMaxMaterials];
  std::vector<double> q(n);
  std::vector<int> small, large;
  for (int s = 0; s < n; ++s) {
    q[s] = F > 0.0 ? (double)H.mat.fco[m + s * kMaxMaterials] * n / F : 1.0;
    (q[s] < 1.0 ? small : large).push_back(s);
    cut[s * nmat + mc] = 1.0f;
    alias[s * nmat + mc] = (unsigned char)s;
  }
  while (!small.empty() && !large.empty()) {
    const int a = small.back(), b = large.back();
    small.pop_back();
    cut[a * nmat + mc] = (float)q[a];
    alias[a * nmat + mc] = (unsigned char)b;
    q[b] -= 1.0 - q[a];
    if (q[b] < 1.0) { large.pop_back(); small.push_back(b); }
  }
}

// Rayleigh and Compton tables per compact material, the shell alias table and the COMPAT kernel's S0 bounds, into TrackCold
static void upload_interaction_tables(const HostModel& H, DeviceModel& D) {
  const int nmat = D.nmat;
  std::vector<float> xco(kRayleighPoints * nmat), pco(xco), aco(xco), bco(xco);
  std::vector<unsigned char> itl(kRayleighPoints * nmat), itu(itl);
  std::vector<float> fco(kMaxShells * nmat, 0.f), uico(fco), fj0(fco);
  std::vector<int> nosc(std::max(nmat, 1), 0);
  std::vector<float> shell_cut(kMaxShells * std::max(nmat, 1), 1.0f);
  std::vector<unsigned char> shell_alias(kMaxShells * std::max(nmat, 1), 0);
  for (int m = 0; m < kMaxMaterials; ++m) {
    const int mc = D.compact_of[m];
    if (mc < 0) continue;
    for (int i = 0; i < kRayleighPoints; ++i) {
      xco[mc * kRayleighPoints + i] = H.mat.xco[m * kRayleighPoints + i];
      pco[mc * kRayleighPoints + i] = H.mat.pco[m * kRayleighPoints + i];
      aco[mc * kRayleighPoints + i] = H.mat.aco[m * kRayleighPoints + i];
      bco[mc * kRayleighPoints + i] = H.mat.bco[m * kRayleighPoints + i];
      itl[mc * kRayleighPoints + i] = H.mat.itlco[m * kRayleighPoints + i];
      itu[mc * kRayleighPoints + i] = H.mat.ituco[m * kRayleighPoints + i];
    }
    for (int s = 0; s < kMaxShells; ++s) {
      fco[s * nmat + mc] = H.mat.fco[m + s * kMaxMaterials];
      uico[s * nmat + mc] = H.mat.uico[m + s * kMaxMaterials];
      fj0[s * nmat + mc] = H.mat.fj0[m + s * kMaxMaterials];
    }
    nosc[mc] = H.mat.noscco[m];
    shell_alias_table(H, m, mc, nmat, shell_cut.data(), shell_alias.data());
  }
  TrackCold& cold = D.cold_host;
  cold.xco = D.put(xco); cold.pco = D.put(pco); cold.aco = D.put(aco); cold.bco = D.put(bco);
  cold.itl = D.put(itl); cold.itu = D.put(itu);
  cold.fco = D.put(fco); cold.uico = D.put(uico); cold.fj0 = D.put(fj0);
  cold.s0_bounds = D.put(build_s0_bounds(H, D.compact_of, nmat, &cold.s0_emin, &cold.s0_inv_w));  // COMPAT: bounds of S0 per (material, energy bin)
  cold.noscco = D.put(nosc);
  cold.shell_cut = D.put(shell_cut);
  cold.shell_alias = D.put(shell_alias);
}

static void upload_spectrum(const HostModel& H, DeviceModel& D) {
  TrackCold& cold = D.cold_host;
  cold.espc = D.put(std::vector<float>(H.spectrum.espc, H.spectrum.espc + kMaxSpectrumBins));
  cold.cutoff = D.put(std::vector<float>(H.spectrum.cutoff, H.spectrum.cutoff + kMaxSpectrumBins));
  cold.alias = D.put(std::vector<short>(H.spectrum.alias, H.spectrum.alias + kMaxSpectrumBins));
}

static unsigned short to_half(float f) {  // round to nearest even; inputs are positive normal numbers
  uint32_t x;
  memcpy(&x, &f, 4);
  const int e = (int)((x >> 23) & 0xFF) - 127 + 15;
  uint32_t m = x & 0x7FFFFF;
  if (e <= 0) return 0;
  if (e >= 31) return 0x7BFF;
  uint32_t h = ((uint32_t)e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1FFF;
  if (rem > 0x1000 || (rem == 0x1000 && (h & 1))) ++h;
  return (unsigned short)std::min<uint32_t>(h, 0x7BFF);
}

static double from_half(unsigned short h) { return std::ldexp((double)((h & 0x3FF) | 0x400), (int)(h >> 10) - 25); }

// Brackets of the total cross section for the FAST flight step: per (coarse energy bin = 2^shift table bins, material) the centre
// of [min, max] of a_tot + b_tot * E over the coarse bin as fp16, and per coarse bin one relative half width covering every
// material.  A step whose random number falls outside [1 - m*hi, 1 - m*lo) is decided from LDS alone; only the narrow band in
// between fetches the exact value, so the decisions are those of the exact test.  The LDS image takes the finest table that still
// leaves two workgroups per CU (lay_out_lds_and_brackets).
struct SigmaBrackets {
  std::vector<unsigned short> mid;  // [coarse bin * nmat + mc]
  std::vector<float> w;             // [coarse bin]
};

static SigmaBrackets sigma_brackets(const HostModel& H, const std::vector<float>& tot, int nmat, int shift) {
  const int nv = H.mat.num_values, nc = coarse_bins(nv, shift);
  const double e0 = H.mat.e0, ide = H.mat.ide;
  SigmaBrackets B{std::vector<unsigned short>((size_t)nc * nmat, 0), std::vector<float>(nc, 0.f)};
  for (int c = 0; c < nc; ++c) {
    double wmax = 0.0;
    for (int mc = 0; mc < nmat; ++mc) {
      double lo = 1e300, hi = -1e300;
      for (int i = c << shift; i < std::min(nv, (c + 1) << shift); ++i) {
        const double a = tot[2 * ((size_t)mc * nv + i)], b = tot[2 * ((size_t)mc * nv + i) + 1];
        // the kernel evaluates a + b * E for E in [E_i, E_{i+1}) (one table bin; a little beyond for float rounding)
        const double ea = e0 + (i - 0.01) / ide, eb = e0 + (i + 1.01) / ide;
        lo = std::min(lo, std::min(a + b * ea, a + b * eb));
        hi = std::max(hi, std::max(a + b * ea, a + b * eb));
      }
      if (!(lo > 0.0)) lo = std::min(1e-30, hi > 0.0 ? hi : 1e-30);
      const unsigned short hbits = to_half((float)(0.5 * (lo + hi)));
      B.mid[(size_t)c * nmat + mc] = hbits;
      const double m = from_half(hbits);
      if (hbits == 0 || hbits == 0x7BFF || !(m > 0.0)) { wmax = 1e30; continue; }  // not representable: the band is everything
      wmax = std::max(wmax, std::max((hi - m) / m, (m - lo) / m));
    }
    B.w[c] = (float)std::min(wmax * 1.001 + 1e-5, 1e30);
  }
  return B;
}

// The final LDS image with the finest bracket table that fits kLdsPerWorkgroup (MCGPU_NO_BRACKETS: none), and the brackets
static void lay_out_lds_and_brackets(const HostModel& H, DeviceModel& D, const std::vector<float>& tot) {
  const LdsPlan P = plan_lds(H, D, D.brick_bytes);
  D.sig_shift = -1;
  if (!knob_set("MCGPU_NO_BRACKETS") && D.nmat > 0)
    for (int shift = 6; shift <= 12 && D.sig_shift < 0; ++shift)
      if (lay_out_lds(P, shift).total <= kLdsPerWorkgroup) D.sig_shift = shift;
  D.lds = lay_out_lds(P, D.sig_shift);
  // The cursor table of the staged tally (tally_stage.hpp) takes what the image leaves of the workgroup's LDS -- laid out last, so that
  // neither the brick grid nor the brackets ever give way to it; where it does not fit, this model runs the direct atomics.
  {
    const TallyStagePlan S = tally_stage_plan(4ULL * (unsigned long long)H.detector[0].total_pixels, 1, 1, 0, 0);
    const int bytes = ((int)(S.n_bins + 1u) * 4 + 15) / 16 * 16;
    D.stage.cursor = -1;
    D.stage.bins = 0;
    if (S.n_bins != 0u && D.lds.total + bytes <= kLdsPerWorkgroup) {
      D.stage.cursor = D.lds.total;
      D.stage.bins = S.n_bins;
      D.lds.total += bytes;
    }
  }
  if (D.sig_shift < 0) return;
  const SigmaBrackets B = sigma_brackets(H, tot, D.nmat, D.sig_shift);
  D.cold_host.sig_mid = D.put(B.mid);
  D.cold_host.sig_w = D.put(B.w);
}

// dose tallies (read_input :1868-1893, init_CUDA_device :2636-2657,2694-2720)
static void upload_dose_tallies(const HostModel& H, DeviceModel& D) {
  const SimConfig& cfg = H.cfg;
  if (cfg.flag_material_dose == 1) {
    D.dose_materials = D.put(std::vector<unsigned long long>(2 * kMaxMaterials, 0ULL));
    D.dose_flags |= kDoseMaterials;
  }
  if (cfg.dose_roi[1] > -1) {
    D.dose_roi_voxels = (size_t)(cfg.dose_roi[1] - cfg.dose_roi[0] + 1) * (size_t)(cfg.dose_roi[3] - cfg.dose_roi[2] + 1) *
                        (size_t)(cfg.dose_roi[5] - cfg.dose_roi[4] + 1);
    D.dose_voxels = D.put(std::vector<unsigned long long>(2 * D.dose_roi_voxels, 0ULL));
    D.dose_flags |= kDoseVoxels;
  }
}

// Azimuthal aperture of the beam (the same for every projection: the pose rotates the beam frame, MC-GPU_v1.3.cu:3280-3434)
static void fan_ratio(const HostModel& H, float& lo_out, float& hi_out) {
  lo_out = -3.0e38f;
  hi_out = 3.0e38f;
  bool same = !H.source.empty();
  for (const SourcePose& sp : H.source) same = same && sp.phi_low == H.source[0].phi_low && sp.D_phi == H.source[0].D_phi;
  if (!same) return;
  const double lo = (double)H.source[0].phi_low, hi = lo + (double)H.source[0].D_phi;
  if (lo > 1.0e-3 && hi < 3.14159265358979323846 - 1.0e-3 && hi > lo) {
    const double r_hi = std::cos(lo) / std::sin(lo), r_lo = std::cos(hi) / std::sin(hi);  // cot decreases on (0, pi)
    const double margin = 2.0e-6 * (r_hi - r_lo);
    lo_out = (float)(r_lo + margin);
    hi_out = (float)(r_hi - margin);
  }
}

// The object region (box, elliptic cylinder) and the brick palette of D into its TrackCold image, uploaded when the image is on
// the device and changed.
void refresh_cold_geometry(DeviceModel& D) {
  TrackCold& ch = D.cold_host;
  TrackCold before;
  memcpy(&before, &ch, sizeof ch);
  for (int k = 0; k < 3; ++k) { ch.objbox_lo[k] = D.objbox_lo[k]; ch.objbox_hi[k] = D.objbox_hi[k]; }
  for (int k = 0; k < 2; ++k) { ch.ell_c[k] = D.ell_c[k]; ch.ell_inv[k] = D.ell_inv[k]; }
  for (int c = 0; c < 16; ++c) ch.brick_palette[c] = D.brick_palette[c];
  if (D.cold && memcmp(&before, &ch, sizeof ch) != 0) HIP_TRY(hipMemcpy(D.cold, &ch, sizeof ch, hipMemcpyHostToDevice));
}

// The rest of TrackCold (the table stages have set their pointers) and its device copy
static void upload_cold(const HostModel& H, DeviceModel& D) {
  upload_dose_tallies(H, D);
  TrackCold& cold = D.cold_host;
  cold.bricks = D.bricks;
  cold.wood_coarse = D.wood_coarse;
  cold.woodcock = D.woodcock;
  cold.lds = D.lds;
  cold.dose_voxels = D.dose_voxels;
  cold.dose_materials = D.dose_materials;
  cold.mfp = D.mfp; cold.e0 = H.mat.e0; cold.ide = H.mat.ide;
  for (int k = 0; k < 3; ++k) cold.bbox[k] = H.voxels.size_bbox[k];
  for (int k = 0; k < 6; ++k) cold.dose_roi[k] = H.cfg.dose_roi[k];
  int shells = 0;
  for (int m = 0; m < kMaxMaterials; ++m) {
    const int mc = D.compact_of[m];
    if (mc < 0) continue;
    cold.material_of_compact[mc] = m;
    cold.shell_first[mc] = shells;
    shells += std::min(H.mat.noscco[m], kMaxShells);
  }
  cold.thresh_compton = cold.thresh_rayleigh = cold.thresh_new = cold.flyable_low = cold.swap_batch = cold.trade_slots = -1;  // apply_schedule
  fan_ratio(H, cold.fan_ratio_lo, cold.fan_ratio_hi);
  refresh_cold_geometry(D);
  D.cold = D.put(std::vector<TrackCold>(1, cold));
}

// Build the palette-compressed volume and the compact-material tables and upload everything.
DeviceModel upload_model(const HostModel& H, int device_id, const DeviceVolumeSource* mapped) {
  DeviceModel D{};
  select_device(D, device_id);
  memset(&D.cold_host, 0, sizeof D.cold_host);
  D.nmat = compact_numbering(H, D.compact_of);
  if (mapped) upload_volume_from_device(H, D, *mapped);
  else upload_volume(H, D);
  const std::vector<float> rec = cross_section_records(H, D.compact_of, D.nmat);
  const std::vector<float> tot = total_cross_sections(rec);
  refresh_woodcock(H, D);
  D.mfp = D.put(rec);
  D.mfp_tot = D.put(tot);
  upload_interaction_tables(H, D);
  upload_spectrum(H, D);
  lay_out_lds_and_brackets(H, D, tot);
  upload_cold(H, D);
  D.src_all = D.put(H.source);
  D.det_all = D.put(H.detector);
  D.work_counter = D.put(std::vector<unsigned long long>((size_t)kNumCounters * kCounterStride, 0ULL));
  D.ev_start = D.mem.event(hipEventDefault);
  D.ev_stop = D.mem.event(hipEventDefault);
  apply_schedule(D);
  HIP_TRY(hipDeviceSynchronize());
  return D;
}

void require(bool ok, int code, const char* msg) { if (!ok) throw Error(code, msg); }

// After mcgpu_warp_geometry the voxels exist on the device only; whoever needs them on the host calls this first.
void sync_host_voxels(mcgpu_ctx& C) {
  if (!C.host_voxels_stale) return;
  HostModel& H = C.host;
  DeviceModel& D = C.dev;
  HIP_TRY(hipSetDevice(D.device_id));
  const size_t nvox = H.voxels.count();
  H.voxels.material.resize(nvox);  // a geometry mapped on the device (mcgpu_set_geometry_image) has had no host arrays yet
  H.voxels.density.resize(nvox);
  std::vector<unsigned char> idx(nvox);
  {  // the device volume is tiled (device_model.hpp: tiled_voxel)
    std::vector<unsigned char> tiled(D.vol_bytes);
    HIP_TRY(hipMemcpy(tiled.data(), D.vol, D.vol_bytes, hipMemcpyDeviceToHost));
    const int nx = H.voxels.n[0], ny = H.voxels.n[1], nz = H.voxels.n[2];
    const unsigned int snx = (unsigned int)D.sub_n[0], snxy = (unsigned int)(D.sub_n[0] * D.sub_n[1]);
    for (int z = 0; z < nz; ++z)
      for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) idx[((size_t)z * ny + y) * nx + x] = tiled[tiled_voxel((unsigned)x, (unsigned)y, (unsigned)z, snx, snxy)];
  }
  int mat_of[256];
  float dens_of[256];
  for (int e = 0; e < D.palette_size; ++e) {
    int mc;
    memcpy(&mc, &D.palette_host[2 * e + 1], 4);
    int number = 1;
    for (int m = 0; m < kMaxMaterials; ++m)
      if (D.compact_of[m] == mc) number = m + 1;
    mat_of[e] = number;
    dens_of[e] = D.palette_host[2 * e];
  }
  for (size_t i = 0; i < nvox; ++i) { H.voxels.material[i] = (uint8_t)mat_of[idx[i]]; H.voxels.density[i] = dens_of[idx[i]]; }
  C.host_voxels_stale = false;
}

const void* host_table(mcgpu_ctx& C, const std::string& name, size_t& bytes) {
  HostModel& H = C.host;
  if (name == "voxel_mat_dens") sync_host_voxels(C);
  auto cache = [&](const void* p, size_t n) -> const void* {
    auto& v = C.table_cache[name];
    v.assign((const unsigned char*)p, (const unsigned char*)p + n);
    bytes = n;
    return v.data();
  };
#define DIRECT(vec) do { bytes = (vec).size() * sizeof((vec)[0]); return (const void*)(vec).data(); } while (0)
  if (name == "source_data") DIRECT(H.source);
  if (name == "detector_data") DIRECT(H.detector);
  if (name == "mfp_woodcock") DIRECT(H.mat.woodcock);
  if (name == "woodcock_coarse") {  // what the FAST kernel stages in LDS (LdsLayout::wood), computed from the table above
    const std::vector<float> w = coarse_woodcock(H);
    return cache(w.data(), w.size() * sizeof(float));
  }
  if (name == "mfp_a") DIRECT(H.mat.a);
  if (name == "mfp_b") DIRECT(H.mat.b);
  if (name == "xco") DIRECT(H.mat.xco);
  if (name == "pco") DIRECT(H.mat.pco);
  if (name == "aco") DIRECT(H.mat.aco);
  if (name == "bco") DIRECT(H.mat.bco);
  if (name == "pmax") DIRECT(H.mat.pmax);
  if (name == "itlco") DIRECT(H.mat.itlco);
  if (name == "ituco") DIRECT(H.mat.ituco);
  if (name == "fco") DIRECT(H.mat.fco);
  if (name == "uico") DIRECT(H.mat.uico);
  if (name == "fj0") DIRECT(H.mat.fj0);
#undef DIRECT
  if (name == "s0_bounds") {  // COMPAT kernel: {lo, hi} of S0 per (material number - 1, energy bin), then {emin, 1 / bin width}
    float emin = 0.f, inv_w = 0.f;
    std::vector<float> b = build_s0_bounds(H, nullptr, kMaxMaterials, &emin, &inv_w);
    b.push_back(emin);
    b.push_back(inv_w);
    return cache(b.data(), b.size() * sizeof(float));
  }
  if (name == "noscco") return cache(H.mat.noscco, sizeof H.mat.noscco);
  if (name == "espc") return cache(H.spectrum.espc, sizeof H.spectrum.espc);
  if (name == "espc_cutoff") return cache(H.spectrum.cutoff, sizeof H.spectrum.cutoff);
  if (name == "espc_alias") return cache(H.spectrum.alias, sizeof H.spectrum.alias);
  if (name == "palette") return cache(C.dev.palette_host.data(), C.dev.palette_host.size() * sizeof(float));  // u8 volumes: {density, bits(compact material)} per entry, in palette order
  if (name == "track_cold" && C.has_device) {
    // the TrackCold scalars a restatement of the source, the exterior hop and the tally needs (tests/source_ref.py), read-only, as
    // 19 floats: fan_ratio_lo, fan_ratio_hi, objbox_lo[3], objbox_hi[3], ell_c[2], ell_inv[2], bbox[3], then the homogeneous exterior:
    // 1 if the geometry has one, its density, its material number - 1 and its compact material index (else 0, 0, -1, -1)
    const DeviceModel& D = C.dev;
    const TrackCold& ch = D.cold_host;
    float v[19] = {ch.fan_ratio_lo, ch.fan_ratio_hi, ch.objbox_lo[0], ch.objbox_lo[1], ch.objbox_lo[2], ch.objbox_hi[0], ch.objbox_hi[1], ch.objbox_hi[2],
                   ch.ell_c[0], ch.ell_c[1], ch.ell_inv[0], ch.ell_inv[1], ch.bbox[0], ch.bbox[1], ch.bbox[2], 0.f, 0.f, -1.f, -1.f};
    if (D.vol_kind == kVolU8 && D.has_exterior && 2 * (size_t)D.background + 1 < D.palette_host.size()) {
      int mc;
      memcpy(&mc, &D.palette_host[2 * (size_t)D.background + 1], 4);
      v[15] = 1.f;
      v[16] = D.palette_host[2 * (size_t)D.background];
      v[18] = (float)mc;
      for (int m = 0; m < kMaxMaterials; ++m)
        if (D.compact_of[m] == mc) v[17] = (float)m;
    }
    return cache(v, sizeof v);
  }
  if (C.has_device) {
    // what the FAST flight step reads (track_pool.inc: flight_locate, flight_resolve), downloaded from the device as it stands there
    // (tests/flight_ref.py): the total cross sections, the brackets, the brick grid and the second level as tile records
    const DeviceModel& D = C.dev;
    auto download = [&](const void* dev_ptr, size_t n) -> const void* {
      auto& v = C.table_cache[name];
      v.assign(n, 0);
      bytes = n;
      if (n != 0 && dev_ptr != nullptr) {
        HIP_TRY(hipSetDevice(D.device_id));
        HIP_TRY(hipMemcpy(v.data(), dev_ptr, n, hipMemcpyDeviceToHost));
      }
      return v.data();
    };
    const size_t nc = D.sig_shift >= 0 ? (size_t)coarse_bins(H.mat.num_values, D.sig_shift) : 0;
    if (name == "mfp_tot") return download(D.mfp_tot, (size_t)D.nmat * (size_t)H.mat.num_values * 2 * sizeof(float));  // float2 {a_tot, b_tot} per row mc * num_values + bin
    if (name == "sigma_bracket_mid") return download(D.cold_host.sig_mid, nc * (size_t)D.nmat * 2);  // fp16 words [coarse bin * nmat + mc]; empty: no brackets
    if (name == "sigma_bracket_w") return download(D.cold_host.sig_w, nc * sizeof(float));
    if (name == "compact_of") return cache(D.compact_of, sizeof D.compact_of);  // int[25]: compact material of material number - 1, -1: unused
    if (name == "brick_palette") return cache(D.cold_host.brick_palette, sizeof D.cold_host.brick_palette);  // int[16]: palette index of brick code c
    if (name == "brick_codes") return download(D.vol_kind == kVolU8 ? D.bricks : nullptr, D.vol_kind == kVolU8 ? (size_t)D.brick_bytes : 0);  // two 4-bit codes per byte
    if (name == "tile_record_words")  // uint32[4] {ab, code, mask low, mask high} per tile, in tile_record_index order; empty: no records
      return download(D.tile_rec, D.tile_rec ? (size_t)D.rec_n[0] * D.rec_n[1] * D.rec_n[2] * 8 * sizeof(TileRecord) : 0);
  }
  if (name == "density_max") return cache(H.voxels.density_max, sizeof H.voxels.density_max);
  if (name == "density_nominal") return cache(H.mat.density_nominal, sizeof H.mat.density_nominal);
  if (name == "voxel_size") return cache(H.voxels.voxel_size, sizeof H.voxels.voxel_size);
  if (name == "inv_voxel_size") return cache(H.voxels.inv_voxel_size, sizeof H.voxels.inv_voxel_size);
  if (name == "size_bbox") return cache(H.voxels.size_bbox, sizeof H.voxels.size_bbox);
  if (name == "voxel_mat_dens") {  // reference layout: float2 {material + 0.0001f, density} (MC-GPU_v1.3.cu:2135-2136)
    auto& v = C.table_cache[name];
    const size_t n = H.voxels.count();
    v.resize(n * 8);
    float* f = (float*)v.data();
    for (size_t i = 0; i < n; ++i) { f[2 * i] = (float)(H.voxels.material[i]) + 0.0001f; f[2 * i + 1] = H.voxels.density[i]; }
    bytes = v.size();
    return v.data();
  }
  return nullptr;
}


}  // namespace mcgpu
