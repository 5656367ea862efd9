/*
 * mcgpu_amd.h -- C ABI of the MI355X-native Monte Carlo CBCT projection engine.
 *
 * The reference (IPMI-ICNS-UKE/4d-cbct-mc) exposes NO in-process interface for this path: its
 * boundary is process + files (`mpirun -n <ngpu> MC-GPU_v1.3.x input.in`, cbctmc/mc/simulation.py:187-198;
 * SURVEY.md 8b).  This header factors that executable's main() (docker/mcgpu/MC-GPU_v1.3.cu:377-1214)
 * into entry points with plain pointers and sizes, so the same engine can be driven by
 *   - the drop-in executable `MC-GPU_v1.3.x` (4d-cbct-mc_amd/csrc/main.cpp),
 *   - the Python mirror of cbctmc.mc (ctypes, 4d-cbct-mc_amd/engine.py),
 *   - tests and bench.py.
 * Each entry point cites the reference code it replaces.  All functions return 0 on success or a
 * negative error code (the reference's exit codes: -1 input/GPU, -2 parse/alloc, -3 output);
 * mcgpu_last_error() gives the message (it always contains "ERROR", which is what
 * cbctmc/mc/simulation.py:204 greps the engine log for).  No exceptions cross the ABI.
 * Ownership: the context owns host tables and device tables; callers own image buffers.
 */
#ifndef MCGPU_AMD_H_
#define MCGPU_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcgpu_ctx mcgpu_ctx;

/* Kernel personalities.
 * FAST   : production path -- counter-based per-history RNG streams (Philox4x32-7 seeding a
 *          multiply-with-carry lane generator), gfx950 native transcendental instructions, exactly
 *          n_histories histories; statistically equivalent to the reference (3-sigma per pixel).
 * COMPAT : RANECU leap-frog streams (batch <-> thread mapping of MC-GPU_kernel_v1.3.cu:198,841-894),
 *          the reference CPU-build arithmetic and the portable math of oracle/mcgpu_oracle.c;
 *          integer tallies are bit-identical to the CPU oracle. */
#define MCGPU_MODE_FAST 0
#define MCGPU_MODE_COMPAT 1
/* FAST with scheduler statistics (diagnostic build of the same kernel; see mcgpu_scheduler_stats). Not for timing. */
#define MCGPU_MODE_FAST_STATS 2
/* FAST with the three sub-steps the reference computes in double precision -- rotate_double (MC-GPU_kernel_v1.3.cu:1103-1148),
 * GRAa (:1181-1246), GCOa's cdt1 / costh chain (:1329-1331, :1372, :1427) -- in double here too (32-bit deviates where the
 * reference calls ranecu_double): the production kernel at the reference's arithmetic.  Same scheduling, same streams. */
#define MCGPU_MODE_FAST_F64 3

int mcgpu_abi_version(void);
/* The engine's environment knobs as text: one line per knob, tab-separated {name, type (i/f/b/s), scope (K kernel variant or
 * schedule, H host pipeline, T test hook, P Python side), default, current value, description}.  Returns the bytes the whole
 * table needs including the NUL (call with cap = 0 to size a buffer).  No counterpart in the reference (MC-GPU_v1.3.cu reads
 * no environment); `MC-GPU_v1.3.x --knobs` prints it.  A variable MCGPU_* that is not in the table is reported once per
 * process on stdout when a context is created. */
size_t mcgpu_knob_table(char *buf, size_t cap);
const char *mcgpu_last_error(void);

/* read_input + init_energy_spectrum + set_CT_trajectory + load_voxels + load_material
 * (MC-GPU_v1.3.cu:490-562) and, when device_id >= 0, init_CUDA_device (:2454-2724): select the
 * device and upload all tables.  device_id < 0 builds the host model only (no HIP call is made). */
int mcgpu_create(const char *input_path, int device_id, mcgpu_ctx **out);
void mcgpu_destroy(mcgpu_ctx *ctx);
/* A second context of the same simulation on another device (device_id < 0: host only) without parsing the input, the
 * voxel file and the material files again: what each further rank of the reference's `mpirun -n N` repeats in full
 * (MC-GPU_v1.3.cu:377-640: every MPI process runs read_input / load_voxels / load_material).  The clone is independent
 * of `src` afterwards. */
int mcgpu_clone(const mcgpu_ctx *src, int device_id, mcgpu_ctx **out);

/* Scalars parsed from the input file (MC-GPU_v1.3.cu:1280-1615).  Keys: "total_histories", "seed",
 * "gpu_id", "threads_per_block", "histories_per_thread", "num_projections", "enable_specific_angles",
 * "num_voxels_x|y|z", "num_pixels_x|z", "num_materials_used", "num_energy_values", "palette_size",
 * "volume_bytes_device"; of the device model (diagnostic): "volume_kind", "brick_shift", "brick_count", "bricks_mixed",
 * "bricks_exterior", "exterior_cylinder", "exterior_mode" (bit 0: hop across the homogeneous exterior during flight, bit 1: at the source), "tile_records", "sub_brick_table", "fast_scheduler", "segment_loop", "tiles_in_mixed_bricks", "sigma_bracket_shift", "lds_bytes_fast",
 * "lds_bytes_compat", "blocks_per_cu", "num_cus", "device_id". */
int mcgpu_config_i64(const mcgpu_ctx *ctx, const char *key, long long *value);
/* Keys: "D_angle", "initial_angle", "angularROI_0", "angularROI_1", "SRotAxisD", "vertical_translation",
 * "mean_energy_spectrum", "e0", "ide". */
int mcgpu_config_f64(const mcgpu_ctx *ctx, const char *key, double *value);

/* Host tables in the reference's own layouts (MC-GPU_v1.3.h:155-264), for cross-checks against the
 * reference/oracle: "source_data" (80 B x nproj), "detector_data" (100 B x nproj), "voxel_mat_dens"
 * (float2 x nvox, built on demand), "mfp_woodcock", "mfp_a", "mfp_b", "xco","pco","aco","bco","pmax",
 * "itlco","ituco","fco","uico","fj0","noscco","espc","espc_cutoff","espc_alias","density_max",
 * "density_nominal","voxel_size","inv_voxel_size","size_bbox"; of the device model: "palette" (float2 {density, bits(compact material
 * index)} per entry of a u8 palette volume, in palette order), "track_cold" (contexts with a device; 19 floats the FAST kernels read at their
 * scheduling points: fan_ratio_lo, fan_ratio_hi, object box lo[3] / hi[3], elliptic cylinder centre[2] / inverse squared semi-axes[2] (0: none),
 * bounding box[3], then the homogeneous exterior: 1 if there is one, its density, its material number - 1, its compact material index);
 * contexts with a device, what the FAST flight step reads, downloaded from the device: "mfp_tot" (float2 {a, b} of the total cross section
 * per row compact material * num_energy_values + bin), "sigma_bracket_mid" (fp16 words [coarse bin * materials used + compact material]) and
 * "sigma_bracket_w" (float per coarse bin of 2^sigma_bracket_shift bins; both empty without brackets), "compact_of" (int[25]: compact
 * material of material number - 1, -1 unused), "brick_codes" (two 4-bit codes per byte, brick x fastest; u8 volumes), "brick_palette"
 * (int[16]: palette index of brick code c), "tile_record_words" (uint32[4] {entries, code, mask low, mask high} per 4x4x4 tile, eight
 * tiles of a 2x2x2 cube contiguous; empty without tile records).
 * The pointer stays valid until destroy. */
int mcgpu_host_table(mcgpu_ctx *ctx, const char *name, const void **data, size_t *bytes);

/* Output file name of projection p: "<base>_%010.6fdeg" with the float32 angle (MC-GPU_v1.3.cu:2787-2803). */
int mcgpu_projection_file_name(const mcgpu_ctx *ctx, int p, char *buf, size_t buf_bytes);

/* Number of uint64 tally words per projection: 4 * Nx * Nz (MC-GPU_v1.3.cu:1848-1849). */
int mcgpu_image_words(const mcgpu_ctx *ctx, size_t *words);

/* Launch sizing of the reference (MC-GPU_v1.3.cu:823-841): blocks of `threads` threads, `hpt`
 * histories per thread (raised when blocks would exceed 65535); total = blocks*threads*hpt. */
int mcgpu_launch_shape(unsigned long long histories, int threads_per_block, int histories_per_thread, int *blocks,
                       int *hpt_out, unsigned long long *total_histories);

/* update_seed_PRNG (MC-GPU_v1.3.cu:3456-3485): seed for the next projection. */
int mcgpu_advance_seed(int batch_number, unsigned long long total_histories, int seed);

/* track_particles<<<>>> for projection p (MC-GPU_v1.3.cu:861; kernel MC-GPU_kernel_v1.3.cu:120-384),
 * asynchronous on `hip_stream` (a hipStream_t, NULL = default stream), ADDING into the caller's device
 * buffer image_dev[4*Nx*Nz] (uint64).  History sharding: the launch simulates
 *   FAST  : history ids [first, first+count)            (count = n_histories for a single GPU)
 *   COMPAT: batches     [first, first+count) of `hpt` histories each (batch b uses RANECU stream b)
 * so ranks given disjoint ranges produce images whose sum equals the single-GPU image exactly.
 * `seed` is the RNG seed for this projection; `hpt` is ignored in FAST mode. */
int mcgpu_launch_projection(mcgpu_ctx *ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count,
                            int hpt, void *image_dev, void *hip_stream);
/* The same launch with a second tally beside the image: w2_dev[4*Nx*Nz] (uint64, the image's layout), ADDED into like the image.  A
 * history that scores w (round(E * 100), 0.01 eV) in word i also adds (w >> 10)^2 to w2[i] -- the sum of squared weights in units of
 * (1024 * 0.01 eV)^2, from which mcgpu_finalize_variance gives the variance of every pixel of the projection out of the one run that is
 * made anyway.  All modes; the image is bit for bit the one of the launch without w2; disjoint ranges sum as the image's do.  No
 * sum can overflow (a term is at most 1.5e8); the shift costs at most 0.4 % of a term at the 5 keV table floor, 0.03 % at the mean
 * energy.  A FAST launch with w2 stages its hits wherever the detector has a staging plan (MCGPU_TALLY_STAGE=0 still forces the direct
 * atomics).  w2_dev == NULL is mcgpu_launch_projection. */
int mcgpu_launch_projection_w2(mcgpu_ctx *ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count,
                               int hpt, void *image_dev, void *w2_dev, void *hip_stream);
/* Staged detector tally of the FAST kernels (csrc/tally_stage.hpp; MCGPU_TALLY_STAGE): hits are stored per (workgroup, bin) and a
 * second kernel folds them into the image, inside the launch's events.  The plan for a detector of `detector_words` tally words
 * (4 * Nx * Nz), a launch of `histories` cut into sub-launches of at most `limit`, and `workgroups` workgroups; `bins` = 0: the
 * engine's choice.  out6 = {bins (0: no staging), words per bin, pixels per bin, records per (workgroup, bin), bytes of the
 * staging buffer = capacity * workgroups * bins * 8, sub-launches}.  Host arithmetic only: `ctx` may be NULL or have no device. */
int mcgpu_tally_stage_plan(const mcgpu_ctx *ctx, unsigned long long detector_words, unsigned long long histories, int workgroups,
                           int bins, unsigned long long limit, unsigned long long *out6);
/* Test support (no caller in the engine or the drop-in needs these two; they exist so that the mapping and the split the kernels use
 * can be checked on a machine without a GPU).  Tally words first .. first+n-1 -> their bin and bin-relative word under that plan. */
int mcgpu_tally_stage_map(unsigned long long detector_words, int bins, unsigned long long first, unsigned long long n,
                          unsigned int *bin_out, unsigned int *rel_out);
/* History range of sub-launch k of a staged launch of [first, first+count) at sub-launch limit `limit`. */
int mcgpu_tally_stage_sub_launch(unsigned long long first, unsigned long long count, unsigned long long limit, unsigned long long k,
                                 unsigned long long *sub_first, unsigned long long *sub_count);
/* How a FAST launch of `count` histories deals its ids: tickets first_ticket .. first_ticket+n-1 of id dispenser `counter`
 * (0..63) are the ids lo_out[i] .. hi_out[i]-1 of the launch (relative to its first history; lo == hi: the dispenser is exhausted).
 * *n_tickets (may be NULL): the dispenser's non-empty tickets.  Pure host arithmetic, the functions the kernels use. */
int mcgpu_id_tickets(unsigned long long count, int counter, unsigned long long first_ticket, unsigned long long n,
                     unsigned long long *lo_out, unsigned long long *hi_out, unsigned long long *n_tickets);
/* The dispenser a wave asks after `counter` when `mask` holds a bit for every dispenser reported exhausted: the first one after
 * it, cyclically, whose bit is clear; 64 when none is; -1 for a bad `counter`. */
int mcgpu_id_next_counter(unsigned long long mask, int counter);
/* Milliseconds between the HIP events recorded around the most recent launch on its stream
 * (synchronises on the stop event). */
int mcgpu_last_kernel_ms(mcgpu_ctx *ctx, float *ms);
/* Scheduler statistics accumulated by MCGPU_MODE_FAST_STATS launches: out8 = {wave loop iterations, sum of flying
 * lanes, Compton rounds, Compton lanes, Rayleigh rounds, Rayleigh lanes, tally+source rounds, their lanes}. */
int mcgpu_scheduler_stats(mcgpu_ctx *ctx, unsigned long long *out8, int reset);
/* Batching thresholds of the FAST kernel, in lanes of a wave64: pending Compton / Rayleigh / tally+source histories that
 * trigger a batch, the number of lanes able to fly below which every well-populated kind is served, and how many lanes park
 * between two scheduling points.  Results never depend on them (per-history RNG streams, integer tallies); speed does, by a
 * few percent between geometries.  mcgpu_run_scan picks among a few presets with short throw-away launches unless
 * MCGPU_THRESH_* / MCGPU_FLYABLE_LOW / MCGPU_SWAP_BATCH are set in the environment (those always win). */
int mcgpu_set_fast_schedule(mcgpu_ctx *ctx, int thresh_compton, int thresh_rayleigh, int thresh_new, int flyable_low, int swap_batch);
/* The tuning knobs of the environment (MCGPU_THRESH_*, MCGPU_FLYABLE_LOW, MCGPU_SWAP_BATCH, MCGPU_SLOT_TRADE,
 * MCGPU_HOLD_Q, MCGPU_EXTERIOR_MODE, MCGPU_BLOCKS_PER_CU, MCGPU_GRID_SPARE_PERCENT, MCGPU_COMPAT_THRESH_*) are read ONCE, when
 * the context's device model is built; mcgpu_launch_projection never reads the environment and never synchronises.  Tuning
 * tools that change them in a live process call this to read them again (drains the device, re-uploads the parameter block).
 * The reference has no counterpart: its launch shape is fixed by the input file (MC-GPU_v1.3.cu:823-841). */
int mcgpu_reload_env_knobs(mcgpu_ctx *ctx);
/* The same with the full counter set (up to 16): 8 = scheduling points, 9/10 = register<->LDS-slot exchange rounds /
 * lanes that bring a flying history in, 11 = scheduling points in drain mode. */
int mcgpu_scheduler_stats_ex(mcgpu_ctx *ctx, unsigned long long *out, int capacity, int reset);
/* Convenience for callers without a HIP binding of their own (ctypes hosts, tests): copy `bytes` from device memory of the
 * context's device to host memory, ordered behind everything enqueued on `hip_stream` so far; returns when the data is there. */
int mcgpu_copy_to_host(mcgpu_ctx *ctx, const void *src_dev, void *dst_host, size_t bytes, void *hip_stream);

/* hipMemsetAsync of an image buffer (init_image_array_GPU, MC-GPU_kernel_v1.3.cu:56-72). */
int mcgpu_clear_image(mcgpu_ctx *ctx, void *image_dev, void *hip_stream);

/* Convenience, synchronous: allocate+zero a device image, launch, wait, copy to image_host[4*Nx*Nz]
 * (MC-GPU_v1.3.cu:861-907).  kernel_seconds / histories_done may be NULL. */
int mcgpu_run_projection(mcgpu_ctx *ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                         uint64_t *image_host, double *kernel_seconds, unsigned long long *histories_done);

/* The same with the squared weights of mcgpu_launch_projection_w2 copied to w2_host[4*Nx*Nz] (NULL: mcgpu_run_projection). */
int mcgpu_run_projection_w2(mcgpu_ctx *ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                            uint64_t *image_host, uint64_t *w2_host, double *kernel_seconds, unsigned long long *histories_done);

/* report_image (MC-GPU_v1.3.cu:2783-2953): write the ASCII projection file (file_name NULL = the
 * reference's name for projection p).  Values = image * (1/100) * inv_px_X * inv_px_Z / total_histories. */
int mcgpu_write_projection(mcgpu_ctx *ctx, int p, const uint64_t *image_host, unsigned long long total_histories, double seconds,
                           const char *file_name);

/* report_image with the 1.4 M data lines formatted ON THE DEVICE (MC-GPU_v1.3.cu:2860-2904: four "%.8lf" numbers per pixel,
 * a blank line per detector row; exact decimal conversion in integer arithmetic, byte-identical to mcgpu_write_projection).
 * mcgpu_format_projection is asynchronous on `hip_stream`: it reads the device tally `image_dev` (before it is cleared) and
 * fills one of MCGPU_ASCII_SLOTS internal slots and records an event behind it; the host side
 * mcgpu_write_formatted_projection waits for that event, downloads the text with a copy engine and writes header + text +
 * footer.  A tally with a value outside the formatter's range (>= 1e11 eV/cm^2 per history; unreachable for photon physics)
 * makes it return -3 -- there is no host fallback on this route (the tally has been cleared by then).  The scan driver
 * cycles through the slots with one writer thread each, so the files of projections i - 2 .. i are written side by side
 * while i + 1 is tracked and formatted.  Different slots may be used from different threads at the same time. */
#define MCGPU_ASCII_SLOTS 3
int mcgpu_format_projection(mcgpu_ctx *ctx, const void *image_dev, unsigned long long total_histories, int slot, void *hip_stream);
int mcgpu_write_formatted_projection(mcgpu_ctx *ctx, int p, int slot, unsigned long long total_histories, double seconds,
                                     const char *file_name);

/* Dose tallies (tally_materials_dose MC-GPU_kernel_v1.3.cu:1547-1563, tally_voxel_energy_deposition :418-443; enabled by
 * SECTION DOSE DEPOSITION of the input file, MC-GPU_v1.3.cu:1619-1709).  The context owns device buffers that every
 * launch adds into (all projections accumulate, as in the reference).
 *   flags: bit 0 = material dose tally, bit 1 = voxel dose tally; roi6 = 0-based inclusive xmin,xmax,ymin,ymax,zmin,zmax;
 *   voxels: uint64 pairs {Edep*100, Edep^2} per ROI voxel (x fastest); materials: uint64 pairs x 25 material numbers. */
int mcgpu_dose_info(const mcgpu_ctx *ctx, int *flags, int roi6[6], size_t *roi_voxels);
int mcgpu_dose_read(mcgpu_ctx *ctx, uint64_t *voxels_out /* 2*roi_voxels or NULL */, uint64_t *materials_out /* 50 or NULL */);
int mcgpu_dose_clear(mcgpu_ctx *ctx);
/* report_voxels_dose (MC-GPU_v1.3.cu:2976-3199: ASCII z-plane file + <file>.raw + <file>_2sigma.raw) when `voxels` is
 * given, report_materials_dose (:3214-3262) when `materials` is given.  The text the reference prints to stdout goes to
 * `log` (NUL-terminated, truncated to log_bytes) or, when log is NULL, to stdout. */
int mcgpu_write_dose_report(mcgpu_ctx *ctx, const uint64_t *voxels, const uint64_t *materials, unsigned long long histories_per_projection,
                            double seconds, char *log, size_t log_bytes);

/* ---- projection post-processing and RTK-ready stacks (cbctmc/mc/projection.py:36-169, simulation.py:235-277) ----
 * The reference's Python reads every ASCII projection back (np.loadtxt -> float32), flips z, crops the half-fan columns
 * and stacks {total, unscattered, scattered} into MetaImage files.  These entry points produce the same float32 numbers
 * from the integer tallies directly.  planes = float[3][Nz][crop_nx] (total, unscattered, scattered); crop_nx <= 0 or
 * >= Nx keeps the full width. */
int mcgpu_finalize_projection(mcgpu_ctx *ctx, void *image_dev, unsigned long long total_histories, int crop_nx, void *planes_dev,
                              int clear_image, void *hip_stream);
int mcgpu_finalize_projection_host(const mcgpu_ctx *ctx, const uint64_t *image_host, unsigned long long total_histories, int crop_nx,
                                   float *planes_host);
/* Per-pixel variance of those planes from the image and the squared weights tallied beside it (mcgpu_launch_projection_w2): same
 * flip, crop and plane order.  Per pixel and plane, with W the sum of the plane's image words, Q the sum of its w2 words, N =
 * total_histories and c = (1/100) * inv_px_X * inv_px_Z:
 *     var = c^2 * (1048576 * Q - W * W / N) / (N * (N - 1))
 * in double, in that order, as float32 -- the unbiased estimate of the variance of the value the plane reports; negative results
 * are 0, N < 2 gives 0.  The device kernel and the host function agree bit for bit.  clear_w2 zeroes w2 in the same pass (the image is
 * only read). */
int mcgpu_finalize_variance(mcgpu_ctx *ctx, const void *image_dev, void *w2_dev, unsigned long long total_histories, int crop_nx,
                            void *planes_dev, int clear_w2, void *hip_stream);
int mcgpu_finalize_variance_host(const mcgpu_ctx *ctx, const uint64_t *image_host, const uint64_t *w2_host,
                                 unsigned long long total_histories, int crop_nx, float *planes_host);
/* MetaImage float32 stack written plane by plane (projections_to_itk, projection.py:118-166: spacing (sx, sy, 1), origin
 * (-nx*sx/2, -ny*sy/2, 0)).  finish(replace_zeros != 0) applies np.where(stack == 0, stack[stack > 0].min(), stack). */
typedef struct mcgpu_stack mcgpu_stack;
int mcgpu_stack_create(const char *path, int nx, int ny, int nslices, double spacing_x, double spacing_y, mcgpu_stack **out);
int mcgpu_stack_append(mcgpu_stack *stack, const float *plane);
int mcgpu_stack_write_slice(mcgpu_stack *stack, int slice, const float *plane); /* any order, each slice once; not mixed with append */
int mcgpu_stack_finish(mcgpu_stack *stack, int replace_zeros, float *replacement_value);
int mcgpu_stack_read(const char *path, int dims3[3], float *data /* NULL: dims only */, size_t capacity_elements);
/* normalize_projections (projection.py:96-115): out = log(gaussian_filter(air, (sigma_y, sigma_x)) / total), scipy's
 * gaussian_filter semantics (truncate 4, reflect); sigma <= 0 skips the filter. */
int mcgpu_normalize_stack(const char *total_stack, const char *air_stack, double sigma_y, double sigma_x, const char *out_stack,
                          double spacing_x, double spacing_y);

/* Whole-scan driver on the context's GPU: the projection loop of main() (MC-GPU_v1.3.cu:667-1056) as a pipeline --
 * track -> finalize (+ clear) on the device, double-buffered pinned copies, a writer thread for the files -- so the GPU
 * never waits for output.  Zero-initialise the struct, THEN set struct_size = sizeof(mcgpu_scan_options); every other field has a
 * usable default.  struct_size stays the first field for good: inserting anything before it would be a deliberate ABI break. */
typedef struct mcgpu_scan_options {
  /* sizeof(mcgpu_scan_options) as the CALLER was compiled: fields the caller's header did not have yet read as zero (their
   * defaults), instead of whatever follows the shorter struct in memory.  0 is refused. */
  unsigned int struct_size;
  int mode;                                     /* MCGPU_MODE_FAST (default), MCGPU_MODE_FAST_F64 or MCGPU_MODE_COMPAT; any other value is refused */
  int first_projection, num_projections;        /* num_projections 0 = all remaining */
  unsigned long long histories_per_projection;  /* 0 = the input file's value */
  int crop_nx;                                  /* half-fan crop of the stacks (reference default 1024); 0 = full width */
  int write_ascii;                              /* the reference's per-projection ASCII files */
  int write_stacks;                             /* projections_{total,unscattered,scattered}.mha in output_folder */
  const char *output_folder;                    /* NULL = folder of the input file's output base name */
  const char *air_stack;                        /* air scan's projections_total.mha: also write projections_total_normalized.mha */
  double air_sigma_y, air_sigma_x;              /* gaussian denoising of the air projection (reference default 10, 10) */
  double pixel_spacing_x, pixel_spacing_y;      /* MetaImage spacing [mm]; 0 = detector pixel size of the input file */
  /* 4-D scans: three caller-owned stacks {total, unscattered, scattered} shared by several scans; projection i of THIS
   * scan (i = 0 .. num_projections-1) is written to slice slice_of_projection[i].  The caller finishes the stacks. */
  mcgpu_stack **shared_stacks;
  const int *slice_of_projection;
  int progress;                                 /* print the reference's "<< Simulating Projection i of n >>" lines to stdout */
  /* mcgpu_run_scan_multi: how the work is split over the contexts.  MCGPU_SHARD_HISTORIES (0, default): the reference's split
   * (every projection's histories over the devices, tallies summed; MC-GPU_v1.3.cu:728-731, :1019).  MCGPU_SHARD_PROJECTIONS:
   * context g simulates ALL histories of the simulated projections number g, g + n, g + 2n, ... and nothing crosses between the
   * devices (SURVEY.md 8e's fallback: no exchange, no collective); outputs are identical to a one-device scan. */
  int shard;
  /* simulate only the simulated projections number phase, phase + stride, ... of the range (0, 0 = all): what
   * MCGPU_SHARD_PROJECTIONS hands to each context; usable directly by a host that runs one mcgpu_run_scan per device */
  int projection_stride, projection_phase;
  /* mcgpu_run_scan_multi with MCGPU_SHARD_HISTORIES: how the per-device tallies of a projection are summed (the reference's
   * MPI_Reduce, MC-GPU_v1.3.cu:1006-1024).  MCGPU_REDUCE_AUTO (0): the tally exchange; where the devices cannot reach each other,
   * projection sharding (no RCCL in between) -- unless the environment says MCGPU_REDUCE=rccl, which makes it MCGPU_REDUCE_RCCL.
   * MCGPU_REDUCE_RCCL: one ncclReduce(uint64, sum, root = the projection's owner) per projection on a stream of
   * its own beside the next projection's kernel (then projection sharding if RCCL cannot be set up).  Same output bytes on every route. */
  int reduce;
  /* mcgpu_run_scan with write_stacks: every projection also tallies its squared weights (mcgpu_launch_projection_w2; kept directly
   * behind the image in one allocation) and projections_{total,unscattered,scattered}_variance.mha are written beside the stacks
   * (mcgpu_finalize_variance; same spacing, no zero replacement).  Every other output keeps its bytes.  Refused (-1) without
   * write_stacks, with shared_stacks and by mcgpu_run_scan_multi. */
  int write_variance;
} mcgpu_scan_options;
#define MCGPU_SHARD_HISTORIES 0
#define MCGPU_SHARD_PROJECTIONS 1
#define MCGPU_REDUCE_AUTO 0
#define MCGPU_REDUCE_RCCL 1
typedef struct mcgpu_scan_report {
  int projections;
  unsigned long long histories_per_projection;
  double seconds_total, seconds_kernels, seconds_after_last_kernel;
  float zero_replacement[3];
  double seconds_writer;                        /* busy time of the output thread (overlapped with tracking) */
  double kernel_ms_min, kernel_ms_max;          /* fastest / slowest projection of the scan (the slowest device's launch each): kernels vary with the angle */
} mcgpu_scan_report;
int mcgpu_run_scan(mcgpu_ctx *ctx, const mcgpu_scan_options *options, mcgpu_scan_report *report);
/* The same over several devices of one node (contexts created from the same input file, one per device): every
 * projection's histories are sharded over the contexts (the reference's `mpirun -n N`, MC-GPU_v1.3.cu:728-731,823-841) and the
 * per-device tallies are summed through the tally exchange below (the MPI_Reduce of :1019): every projection has an owner
 * device (projection mod devices; MCGPU_EXCHANGE_POLICY=0: always the first), the others push their tally to it with a copy
 * engine beside their next kernel, the owner adds them in one pass, finalizes, formats and downloads the projection; the
 * writer thread takes the results in projection order.  No device waits for the sum.  Dose tallies stay per context (sum
 * them with mcgpu_dose_read). */
int mcgpu_run_scan_multi(mcgpu_ctx *const *ctxs, int n_ctx, const mcgpu_scan_options *options, mcgpu_scan_report *report);

/* ---- The tally exchange between the GPUs of one node: the sum of the per-rank detector tallies that the reference does with
 * a device-to-host copy and a blocking MPI_Reduce to rank 0 per projection (MC-GPU_v1.3.cu:1006-1024).  One mcgpu_exchange
 * per rank -- a process with its own GPU (bench.py, one process per GPU) or a context of one process
 * (mcgpu_run_scan_multi) -- all built over one small host region `shared` of mcgpu_exchange_shared_bytes(world) ZEROED bytes
 * that every rank sees (plain memory inside one process, a mapped /dev/shm file between processes).  Every step
 * (projection) has an owner rank: policy 0 = rank 0, MCGPU_EXCHANGE_ROTATE = step mod world.  Per step, on the rank's
 * tracking stream:   begin(step) -> tally buffer (zeroed) | mcgpu_launch_projection into it | submit(step) |
 * collect(step - 1).  submit: a rank that does not own the step pushes its tally into the owner's landing buffer with a COPY
 * ENGINE (no kernel may run beside the persistent tracking grid), overlapped with the next projection's tracking.
 * collect: the owner adds the landed tallies to its own in one fused pass behind its next kernel and gets the complete
 * tally (valid until begin(step + 2)); other ranks get NULL.  Integer sums: the result equals the single-GPU tally bit for
 * bit.  Between processes ranks swap "cards" (IPC memory and event handles) once: card() on every rank, an all-gather by
 * whatever means the host has (its process-group library, MPI, a file), connect() to every peer.  A rank that waits for a peer
 * that has gone gets an error after 120 s, never a hang. */
typedef struct mcgpu_exchange mcgpu_exchange;
#define MCGPU_EXCHANGE_ROTATE 1 /* policy bit: owner of step s is rank s % world (default: rank 0, the reference's root) */
#define MCGPU_EXCHANGE_LOCAL 2  /* policy bit: every rank is a context of THIS process (plain events, connect_local) */
size_t mcgpu_exchange_shared_bytes(int world);
size_t mcgpu_exchange_card_bytes(int world);
int mcgpu_exchange_create(int device_id, int rank, int world, size_t words, int policy, void *shared, mcgpu_exchange **out);
int mcgpu_exchange_card(mcgpu_exchange *x, unsigned char *card, size_t card_bytes);
int mcgpu_exchange_connect(mcgpu_exchange *x, int peer, const unsigned char *card, size_t card_bytes);
int mcgpu_exchange_connect_local(mcgpu_exchange *x, mcgpu_exchange *peer);
/* after all peers are connected, before the first step: one small copy-engine transfer into every peer's landing buffer, waited
 * for -- a platform without that path between two devices fails here, where the ranks can still agree on another route */
int mcgpu_exchange_probe(mcgpu_exchange *x);
int mcgpu_exchange_owner(const mcgpu_exchange *x, long long step);
int mcgpu_exchange_begin(mcgpu_exchange *x, long long step, void *hip_stream, void **tally_dev);
int mcgpu_exchange_submit(mcgpu_exchange *x, long long step, void *hip_stream);
int mcgpu_exchange_collect(mcgpu_exchange *x, long long step, void *hip_stream, void **reduced_dev);
/* out6 = {last push [ms], last fused add [ms], pushes, collects, host seconds spent waiting for peers, bytes per push} */
int mcgpu_exchange_stats(mcgpu_exchange *x, double out6[6]);
void mcgpu_exchange_destroy(mcgpu_exchange *x);

/* The vendor-collective route of the same sum (reduce_rccl.cpp): one communicator per device of this process (ncclCommInitAll),
 * then per projection ONE ncclReduce(uint64, sum, root) of the devices' tallies -- the reference's MPI_Reduce(MPI_UNSIGNED_LONG_LONG,
 * MPI_SUM, root 0) of MC-GPU_v1.3.cu:1019 without the trip through the host.  RCCL is opened on first use (dlopen), never linked.
 * create: 0, or -1 when the route cannot be taken here (no library, a device listed twice, no path between the devices) with the
 * reason in mcgpu_last_error().  reduce: tallies[g] is uint64[words] on device g; the sum lands in tallies[root]; the call is
 * enqueued on hip_streams[g] (one thread drives all devices: one group). */
typedef struct mcgpu_rccl mcgpu_rccl;
int mcgpu_rccl_create(const int *devices, int n, mcgpu_rccl **out);
int mcgpu_rccl_reduce_u64(mcgpu_rccl *r, void *const *tallies, size_t words, int root, void *const *hip_streams);
void mcgpu_rccl_destroy(mcgpu_rccl *r);

/* Replace the context's geometry by warp(base geometry, displacement) WITHOUT leaving the device: what
 * MCSimulation4D does per respiratory state with `MCGeometry.warp` + a new voxel file + a new engine process
 * (cbctmc/mc/simulation.py:643-692, cbctmc/mc/geometry.py:386-439).  The base geometry is the one resident at the first
 * call.  displacement: host floats in voxels; frame 0: [3][nz][ny][nx] in the engine's frame (components x, y, z); frame 1:
 * [3][gx][gy][gz] in the frame of the reference's MCGeometry arrays, of which the engine volume is the rot90(k=3) in the x/y
 * plane (cbctmc/mc/geometry.py:589-599) -- the field CorrespondenceModel.predict returns, as it is.  Nearest neighbour with
 * the float32 arithmetic of the grid_sample(nearest, align_corners=True) the reference calls, evaluated in the field's own frame
 * (tests/golden/warp_kat.npz); voxels sampled from outside get (default_material,
 * default_density), which must be in the palette (air at 0.0013 always is).  Palette index volume, both brick levels, the
 * object box and the Woodcock majorant are rebuilt on the device (+ a 24001-entry table on the host); needs a palette
 * volume (<= 256 (material, density) pairs), else -5: fall back to mcgpu_warp_volume + mcgpu_set_geometry_arrays.
 * Dose tallies keep accumulating across such changes. */
int mcgpu_warp_geometry(mcgpu_ctx *ctx, const float *displacement, int frame, int default_material, float default_density);

/* ---- The correspondence model resident on the device: the reference's CorrespondenceModel (cbctmc/registration/correspondence.py:
 * 29-226), which turns a breathing signal s[K] into a displacement field, field = mean + coefficients (s - mean_signal), 3N
 * elements for N voxels.  The reference predicts in numpy per respiratory state and warps the result; with the model here a
 * state change sends K doubles and the field is evaluated inside the warp kernel (csrc/correspondence.hip), never stored.
 * Layouts: mean [3N] float or double (mean_is_f64), coefficients double[3N][K] as the reference keeps them, element e = c N + f,
 * c the component and f the voxel of frame 0 ([nz][ny][nx]) or frame 1 ([gx][gy][gz]) as for mcgpu_warp_geometry; N is the
 * context's voxel count.  The field of a signal is float(double(mean[e]) + (coefficients[e][0] d[0] + coefficients[e][1] d[1] + ...)),
 * d = s - mean_signal, summed left to right in double without fused multiply-add.  Device memory: 3N (4 or 8) + 3N K 8 bytes,
 * owned by the context's device model: released by _clear, by a later _set / _fit (also one that fails: then no model is
 * resident), by mcgpu_set_geometry_arrays / mcgpu_set_geometry_image and with the context; a clone does not inherit it.
 * Return codes: 0; -1 bad argument (also: K is not the resident model's); -5 take the host route (predict on the host +
 * mcgpu_warp_geometry, or fit on the host): K > 4, T > 64, no model resident, and for _warp_geometry_signal whatever makes
 * mcgpu_warp_geometry return -5 (no palette volume, default not in the palette).
 * mcgpu_correspondence_set: upload a fitted model (replaces CorrespondenceModel.load + keeping the arrays on the host).
 * mcgpu_correspondence_fit: the large part of CorrespondenceModel.fit (:172-202): fields[t] are T <= 64 host arrays of [3][N]
 *   floats, pinv the T x K pseudo-inverse of the centred signals computed on the host; per element v, in this order of operations,
 *   mean[v] = float((sum_t double(u_t[v])) / T) and coefficients[v][k] = sum_t (double(u_t[v]) - double(mean[v])) pinv[t][k].
 *   The fields pass through the device in slabs of elements (MCGPU_CORRESPONDENCE_SLAB); the results are written into the
 *   resident model's buffers (float mean) and, where the pointers are not null, copied to mean_out [3N] and coefficients_out [3N][K].
 * mcgpu_correspondence_predict: the field of `signal` as float [3][N] in the model's frame (CorrespondenceModel.predict, :206-226).
 * mcgpu_warp_geometry_signal: mcgpu_warp_geometry with the field of `signal` evaluated from the resident model, in the frame the
 *   model was set with: no field crosses the bus and none is stored.
 * mcgpu_correspondence_clear: release the model (0 also when none is resident). */
int mcgpu_correspondence_set(mcgpu_ctx *ctx, const void *mean, int mean_is_f64, const double *coefficients, const double *mean_signal, int K, int frame);
int mcgpu_correspondence_fit(mcgpu_ctx *ctx, const float *const *fields, int T, const double *pinv, const double *mean_signal, int K, int frame,
                             float *mean_out, double *coefficients_out);
int mcgpu_correspondence_predict(mcgpu_ctx *ctx, const double *signal, int K, float *field_out);
int mcgpu_warp_geometry_signal(mcgpu_ctx *ctx, const double *signal, int K, int default_material, float default_density);
int mcgpu_correspondence_clear(mcgpu_ctx *ctx);

/* ---- 4-D: one resident context for many (geometry, projection angles) jobs (cbctmc/mc/simulation.py:527-710 launches the
 * engine once per respiratory state) ----
 * mcgpu_set_projection_angles: the explicit-angle list of SECTION ANGLES OF PROJ (MC-GPU_v1.3.cu:1484-1533) replaced at run
 *   time; poses are rebuilt as set_CT_trajectory does (:3280-3434) -- pose 0 stays the input file's (:3313), which is why the
 *   reference passes the first angle twice (simulation.py:658-660); skip it with mcgpu_scan_options::first_projection = 1.
 * mcgpu_set_geometry_arrays: replace the voxel volume from arrays ([z][y][x], as mcgpu_write_voxel_file takes them); densities
 *   pass through the "%.6f" of the voxel file, the material tables are rebuilt (their Woodcock majorant depends on the
 *   volume) and everything is uploaded again.
 * mcgpu_warp_volume: nearest-neighbour warp of (material, density) by a displacement field [3][nz][ny][nx] in voxel units,
 *   out[x] = in[rint(x + u(x))], default outside (geometry.py:386-439: nearest-neighbour grid sampling of the vroc package), on the
 *   context's GPU. */
int mcgpu_set_projection_angles(mcgpu_ctx *ctx, int n, const float *angles_deg);
int mcgpu_set_geometry_arrays(mcgpu_ctx *ctx, const int n[3], const float spacing_cm[3], const uint8_t *material, const float *density);
int mcgpu_warp_volume(mcgpu_ctx *ctx, const int n[3], const uint8_t *material, const float *density, const float *displacement,
                      int default_material, float default_density, uint8_t *material_out, float *density_out);

/* ---- Row f8: a CT image and its tissue segmentations -> geometry, on the device (csrc/image_map.hip).  Replaces the reference's
 * MaterialMapperPipeline.create_default_pipeline / execute (cbctmc/mc/geometry.py:237-309; the mappers :35-234) as MCGeometry.from_image
 * calls it (:495-577), and -- for mcgpu_set_geometry_image -- the voxel file and engine start that follow it there.
 * The rule (csrc/image_map.hpp states it in full): classes air, soft_tissue, red_marrow, bone_020, bone_050, bone_100, lung, liver,
 * stomach_intestines, muscle_tissue, adipose, blood = table[0..11]; segmentations[0..7] = body, bone, lung, liver, stomach, muscle, fat,
 * lung vessels (uint8, "> 0" is inside; NULL: that line is skipped); v = image value as float32; thresholds = {150, 300, -900} in the
 * reference.  Later lines overwrite: body -> soft_tissue else air | bone: v < t0 red_marrow, t0 <= v < t1 bone_020, v >= t1 bone_050 or
 * bone_100 on the one-voxel outline of the bone mask (6-neighbour erosion, outside the volume = background) | lung | liver | stomach |
 * muscle | fat | body && v < t2 -> air | vessels -> blood.  A NaN fails every comparison.  A voxel no line touches is unmapped.
 * image_dtype: MCGPU_IMAGE_INT16 or MCGPU_IMAGE_FLOAT32.  The C side knows no material: numbers and densities come from `table`.
 * mcgpu_map_image: the mapping alone on the context's GPU (sibling of mcgpu_warp_volume): arrays [n[2]][n[1]][n[0]] in, material /
 *   density out in the same layout with the table's densities as they are; an unmapped voxel gets (0, 0) and is counted in the report.
 * mcgpu_set_geometry_image: replace the context's geometry by the mapped volume; the context is the one mcgpu_set_geometry_arrays
 *   builds from the host-mapped arrays (palette in first-occurrence order of the [z][y][x] scan with air at 0.0013 appended when absent,
 *   table densities through "%.6f" once each, density_max from the classes that occur, material tables and Woodcock majorant rebuilt)
 *   without a voxel-sized pass on the host: the volume, both brick levels and the tile records are built on the device, the host voxel
 *   arrays are downloaded only when someone asks for them.  n / spacing_cm: the ENGINE's grid (nx, ny, nz).  frame 0: inputs
 *   [nz][ny][nx]; frame 1: inputs [gx][gy][gz] = [ny][nx][nz] in the frame of the MCGeometry arrays, engine voxel (x, y, z) = input
 *   voxel (ny - 1 - y, x, z), as for mcgpu_warp_geometry; the permutation happens on the device.
 *   Errors as mcgpu_set_geometry_arrays: -1 bad argument or no device, -2 unmapped voxels (the message carries their number), a class
 *   that occurs with a material number outside 1..25, a density that prints as 0, or a material without data file; after any error the
 *   context is what it was.  On success a resident correspondence model and the warp base are released, dose tallies restart.
 * report (optional; zero it and set struct_size): per class the voxel count and the smallest linear index at which it occurs (-1:
 *   nowhere; [z][y][x] of the engine's frame, for mcgpu_map_image of the input), unmapped voxels, and timings. */
#define MCGPU_IMAGE_INT16 0
#define MCGPU_IMAGE_FLOAT32 1
#define MCGPU_IMAGE_CLASSES 12
#define MCGPU_IMAGE_SEGMENTATIONS 8
typedef struct mcgpu_image_class {
  int material;   /* MC-GPU material number (position of its data file in the input file, from 1) */
  float density;  /* g/cm^3 */
} mcgpu_image_class;
typedef struct mcgpu_image_map_report {
  unsigned int struct_size;  /* sizeof(mcgpu_image_map_report) as the caller was compiled; smaller than 8 is refused */
  unsigned int reserved;
  unsigned long long count[MCGPU_IMAGE_CLASSES];
  long long first[MCGPU_IMAGE_CLASSES];
  unsigned long long unmapped;
  double ms_kernel;                 /* the mapping kernel (HIP events) */
  double ms_upload;                 /* host time of the copies of image and segmentations to the device */
  double ms_install;                /* mcgpu_set_geometry_image: host time from the kernel's end to the context being ready */
  unsigned long long kernel_bytes;  /* bytes the mapping kernel reads and writes once */
} mcgpu_image_map_report;
int mcgpu_map_image(mcgpu_ctx *ctx, const int n[3], const void *image, int image_dtype, const uint8_t *const segmentations[8],
                    const mcgpu_image_class table[12], const float thresholds[3], uint8_t *material_out, float *density_out,
                    mcgpu_image_map_report *report);
int mcgpu_set_geometry_image(mcgpu_ctx *ctx, const int n[3], const float spacing_cm[3], const void *image, int image_dtype,
                             const uint8_t *const segmentations[8], const mcgpu_image_class table[12], const float thresholds[3], int frame,
                             mcgpu_image_map_report *report);

/* ---- Row f12: a 3-D image to another voxel spacing, on the device (csrc/resample.hip).  Replaces the reference's resample_image_spacing
 * (cbctmc/utils.py:76-102: SimpleITK's Resample with the identity transform, origin and direction unchanged) as MCGeometry.from_image
 * calls it for the CT (linear, default -1000) and for every segmentation file (nearest neighbour, default 0; cbctmc/mc/geometry.py:252-261).
 * The rule (csrc/resample.hpp states it in full, with what is NOT pinned against SimpleITK): arrays [n[0]][n[1]][n[2]], the last axis
 * fastest, one spacing per ARRAY axis.  Per axis, in double: M = nearbyint(N * (os / ns)); c = (i * ns) / os; inside iff -0.5 <= c <
 * N - 0.5, else the default value; nearest: floor(c + 0.5); linear: b = clamp(floor(c), 0, N - 1), b1 = min(b + 1, N - 1), d =
 * max(c - b, 0), lerps a + (b - a) * d along the last axis, then the middle, then the first; double -> float32 rounds, double -> int16 /
 * uint8 clamps and truncates toward zero.  Output element type = input element type.
 * mcgpu_resample_plan: the rule per output index, on the host (no device needed): n_out, and -- each NULL or of n_out[0] + n_out[1] +
 *   n_out[2] entries, axis after axis -- base (b), next (b1), frac (d), nearest (clamped into the axis where the output is outside) and
 *   inside.  Call it with NULL arrays first to learn n_out.
 * mcgpu_resample_volume: host arrays in and out ([n_in] -> [n_out] of the plan), resampled on the context's GPU (sibling of
 *   mcgpu_warp_volume and mcgpu_map_image).
 * mcgpu_set_geometry_image_resampled: mcgpu_set_geometry_image of the RESAMPLED image and segmentations without their passing through
 *   the host: the native arrays are uploaded, the image is resampled linearly with image_default outside, every present segmentation by
 *   nearest neighbour with 0 outside, and the mapping kernel and the install run on those device buffers.  n_in and the spacings (mm)
 *   follow the ARRAYS' axes: frame 0: arrays [nz][ny][nx], spacings (z, y, x); frame 1: arrays [gx][gy][gz] of the MCGeometry frame,
 *   spacings (gx, gy, gz).  The engine's grid is the plan's n_out, its spacing_cm spacing_out_mm / 10 as float, both permuted as for
 *   mcgpu_set_geometry_image.  Errors of either part; after any error the context is what it was.  In image_report ms_upload is 0: the
 *   copies to the device are resample_report's.
 * Errors: -1 before any device call: a null pointer, a struct_size below 8, an unknown dtype or interpolator, a size below 1, a
 *   non-finite or non-positive spacing, an axis of the result that rounds to 0 voxels; -2 before any device call: more than 2^31 - 1
 *   voxels on either side. */
#define MCGPU_IMAGE_UINT8 2 /* accepted by the resampler only */
typedef struct mcgpu_resample_options {
  unsigned int struct_size; /* sizeof(mcgpu_resample_options) as the caller was compiled */
  int n_in[3];              /* the input array's shape, slowest axis first */
  double spacing_in[3];     /* per array axis */
  double spacing_out[3];
  int dtype;                /* MCGPU_IMAGE_UINT8, MCGPU_IMAGE_INT16 or MCGPU_IMAGE_FLOAT32 */
  int interpolator;         /* 0 nearest, 1 linear */
  double default_value;     /* of output voxels outside the input; cast like every result */
} mcgpu_resample_options;
typedef struct mcgpu_resample_report {
  unsigned int struct_size;         /* sizeof(mcgpu_resample_report) as the caller was compiled; smaller than 8 is refused */
  double ms_kernel;                 /* the resampling kernels (HIP events) */
  double ms_upload;                 /* host time of allocating on the device and copying the inputs and the plan there */
  double ms_download;               /* host time of copying the result back (mcgpu_resample_volume) */
  unsigned long long kernel_bytes;  /* bytes of the input and output arrays: what the kernels read and write at least once */
} mcgpu_resample_report;
int mcgpu_resample_plan(const mcgpu_resample_options *options, int n_out[3], int *base, int *next, double *frac, int *nearest,
                        unsigned char *inside);
int mcgpu_resample_volume(mcgpu_ctx *ctx, const mcgpu_resample_options *options, const void *in, void *out, mcgpu_resample_report *report);
int mcgpu_set_geometry_image_resampled(mcgpu_ctx *ctx, const int n_in[3], const double spacing_in_mm[3], const double spacing_out_mm[3],
                                       const void *image, int image_dtype, const uint8_t *const segmentations[8],
                                       const mcgpu_image_class table[12], const float thresholds[3], int frame, double image_default,
                                       mcgpu_image_map_report *image_report, mcgpu_resample_report *resample_report);

/* Voxel geometry writer (cbctmc/mc/voxel_data.pyx:12-72 + mcgpu_geometry.jinja2 header fields):
 * material/density are [z][y][x] contiguous, spacing in cm. */
int mcgpu_write_voxel_file(const char *path, const int n[3], const float spacing_cm[3], const uint8_t *material, const float *density,
                           int gzip);

/* Binary sidecar of a voxel file (`geometry.vox[.gz]` -> `geometry.voxbin`): the arrays the text parse would yield (densities
 * quantised through "%.6f" exactly like cbctmc/mc/voxel_data.pyx:25 + MC-GPU_v1.3.cu:2117), palette-compressed.  mcgpu_create
 * prefers a sidecar that is not older than the text file: a 512^3 volume loads in well under a second instead of the
 * 134 M-line text parse per process launch. */
int mcgpu_write_voxel_binary(const char *path, const int n[3], const float spacing_cm[3], const uint8_t *material, const float *density);

/* Hardware ceilings the measurement prices the FAST kernel against, measured on the context's device (about 20 ms each; SURVEY.md
 * 8d; no reference counterpart).  MCGPU_MICROBENCH_VALU_ISSUE: out[0..2] = vector wave-instructions per ns and SIMD of a dense
 * dependent-FMA kernel at 8 waves/SIMD with 64 active lanes, with lanes 0-31, with 32 lanes spread over the wave.
 * MCGPU_MICROBENCH_ATOMIC_RATE: out[0] = scattered 64-bit atomic adds per second into a detector-sized (45 MB) tally.
 * MCGPU_MICROBENCH_COPY_RATE: out[0] = bytes read + written per second by a streaming copy of 256 MiB (16-byte loads and stores). */
#define MCGPU_MICROBENCH_VALU_ISSUE 0
#define MCGPU_MICROBENCH_ATOMIC_RATE 1
#define MCGPU_MICROBENCH_COPY_RATE 2
int mcgpu_microbench(mcgpu_ctx *ctx, int kind, double *out, int n_out);

/* Device-side known-answer hooks used by the parity tests (each runs a tiny kernel on the context's device). */
int mcgpu_kat_rng(mcgpu_ctx *ctx, int mode, int seed, int batch, int hpt, int n, float *out_f32);
/* Raw 32-bit outputs of the FAST personality's per-history streams (no reference counterpart: the reference's RANECU,
 * MC-GPU_kernel_v1.3.cu:841-894, is the COMPAT personality's).  out_u32[i * n_draws + k] = k-th output of the stream of history
 * ids[i] (ids == NULL: first_id + i) at projection `projection`.  generator 0 = production (Philox4x32-7 seeds a multiply-with-
 * carry lane generator; restated in oracle/fast_rng.py), 1 = Philox4x32-10 per draw (the yardstick of the statistical tests). */
int mcgpu_kat_rng_streams(mcgpu_ctx *ctx, int generator, unsigned int seed, unsigned int projection, unsigned long long first_id,
                          const unsigned long long *ids, int n_ids, int n_draws, uint32_t *out_u32);
int mcgpu_kat_math(mcgpu_ctx *ctx, int n, const double *x, double *out_log, double *out_exp, double *out_sin, double *out_cos);
/* expf as the COMPAT kernel evaluates it (the C library's single-precision algorithm, track_common.inc gl_expf) */
int mcgpu_kat_expf(mcgpu_ctx *ctx, int n, const float *x, float *out_exp);
/* float operations of the COMPAT kernel: op 0 its lean square root, 1 sqrtf, 2 its lean quotient a/b, 3 a/b, 4 shell_pz(a, b, inout) */
int mcgpu_kat_f32(mcgpu_ctx *ctx, int op, int n, const float *a, const float *b, float *inout);
/* Double-precision helpers of MCGPU_MODE_FAST_F64 (csrc/track_fast64.hip), item i -> out8[8 i ..]: sin and cos of
 * 2 pi (u[i] + 1/2) 2^-32; 1 / sqrt(a[i]); sqrt(a[i] / b[i]); cdt1 of MC-GPU_kernel_v1.3.cu:1329 at tau = (float)a[i], E = (float)b[i] 1e5;
 * the direction dir3[3 i ..] rotated by polar cosine c[i] and the azimuth of u[i] (rotate_double, :1103-1148). */
int mcgpu_kat_fast64(mcgpu_ctx *ctx, int n, const uint32_t *u, const double *a, const double *b, const double *c, const float *dir3, double *out8);
/* The scattering samplers of MCGPU_MODE_FAST / MCGPU_MODE_FAST_F64 as the photon kernels run them (csrc/kat_scatter.inc: the service
 * bodies of csrc/track_pool.inc, one event per item), from the per-history stream of mcgpu_kat_rng_streams so that a test can replay
 * every deviate.  in4[4 i ..] = {direction u, v, w, photon energy [eV]}, in_u64[i] = history id, material[i] = material number - 1 (one
 * that the context's geometry holds); the stream is that of (id, seed, stream_key).
 *   MCGPU_KAT_RAYLEIGH  Rayleigh events (GRAa, MC-GPU_kernel_v1.3.cu:1181-1246, one trial per service call)
 *   MCGPU_KAT_COMPTON   Compton events (GCOa, :1287-1515, as the shell-first trials of csrc/track_common.inc)
 *   MCGPU_KAT_ROTATE    MCGPU_MODE_FAST only: rotate_dir alone; in4[4 i + 3] = 1 - cos(theta), in_u64[i] = the 32-bit deviate of the
 *                       azimuth (turn fraction: the float nearest to ((u >> 8) + 1/4) 2^-24), material ignored (may be NULL)
 * out4[4 i ..] = {energy, direction u, v, w} after the event; out_u4[4 i ..] = {service calls, final phase (0 = in flight, 5 = below the
 * tables' lowest energy: absorbed), generator state x, c}. */
#define MCGPU_KAT_ROTATE 0
#define MCGPU_KAT_RAYLEIGH 1
#define MCGPU_KAT_COMPTON 2
int mcgpu_kat_scatter(mcgpu_ctx *ctx, int mode, int kind, int n, unsigned int seed, unsigned int stream_key, const float *in4,
                      const unsigned long long *in_u64, const int *material, float *out4, uint32_t *out_u4);
/* The two ends of a history of MCGPU_MODE_FAST / MCGPU_MODE_FAST_F64 as the photon kernels run them (csrc/kat_history.inc: the functions
 * of csrc/track_pool.inc themselves, one item per thread), under the pose of projection `projection` of the context and from the
 * per-history stream of (id, seed, projection), so that a test can replay every deviate.  Nothing is tallied.
 *   MCGPU_KAT_SOURCE  in_u64[i] = history id (in8 may be NULL): a new history -- spectrum energy, direction in the fan, then the entry
 *                     into the volume: across the homogeneous exterior to the object region where the geometry has one (an interaction
 *                     in the background is classified), else the reference's move_to_bbox (MC-GPU_kernel_v1.3.cu:626-686, :714-805)
 *   MCGPU_KAT_TALLY   in8[8 i ..] = {x, y, z, u, v, w, E, scatter state 0..3} (in_u64 may be NULL): an escaped photon is projected onto
 *                     the detector (tally_image, :482-604)
 *   MCGPU_KAT_HOP     in8[8 i ..] = {x, y, z, u, v, w, E, -}, in_u64[i] = history id: one hop across the homogeneous exterior (geometries
 *                     that have one only: others are refused with -2)
 * out8[8 i ..] = {E, u, v, w, x, y, z, Woodcock majorant mean free path}; out_u8[8 i ..] = {final phase (0 in flight, 1 Compton, 2 Rayleigh,
 * 3 escaped, 4 absorbed, 5 new), energy bin, compact material, scatter state, generator state x, c, tally word (0xFFFFFFFF: none), tally
 * value}.  Refused before any launch: a projection outside the context (-1); an energy outside the cross-section tables, an input
 * that is not a number, a scatter state outside 0..3 (-2). */
#define MCGPU_KAT_SOURCE 0
#define MCGPU_KAT_TALLY 1
#define MCGPU_KAT_HOP 2
int mcgpu_kat_history(mcgpu_ctx *ctx, int mode, int kind, int projection, int n, unsigned int seed, const float *in8,
                      const unsigned long long *in_u64, float *out8, uint32_t *out_u8);
/* The middle of a history of MCGPU_MODE_FAST / MCGPU_MODE_FAST_F64, the Woodcock flight step, as the photon kernels run it
 * (csrc/kat_flight.inc: flight_locate, flight_steps, real_record and classify_real of csrc/track_pool.inc themselves, one item per thread, in
 * the kernel variant the context's launches take: out word `variant` = 0 u8, 1 u16, 2 raw float2, 3 u8 with second-level codes, 4 u8 with
 * tile records).  Nothing is tallied.
 *   MCGPU_KAT_LOOKUP  in8[8 i ..] = {x, y, z, ...} (in_u64 may be NULL, max_steps is ignored): the voxel look-up of a step that ends at that
 *                     point, no deviate drawn.  out_u32[8 i ..] = {bits(density), compact material, brick code or 15 = mixed, voxel's palette
 *                     index (mixed only), 1 if the point was clamped into the volume (outside), 1 if the brick is exterior, variant, 0}
 *   MCGPU_KAT_FLIGHT  in8[8 i ..] = {x, y, z, u, v, w, E, -}, in_u64[i] = history id, max_steps in 1..32: flight steps from that state (energy
 *                     bin and coarse majorant of E, no cached cross section, the stream of (id, seed, projection)) while the history is in
 *                     flight, at most max_steps; a real interaction then draws its kind.  out_u32[(max_steps + 1) 8 i ..] = one row {bits(x),
 *                     bits(y), bits(z), phase (0 in flight, 3 escaped, 7 real, 8 virtual in the exterior), compact material, bits(cached total
 *                     cross section), generator state x, c} after every step taken (the others stay zero), then {final phase (0, 3, 8, or the
 *                     kind: 1 Compton, 2 Rayleigh, 4 absorbed), steps taken, energy bin, bits(majorant mean free path), generator state x, c,
 *                     variant, the compact material whose total cross section is cached (0xFFFFFFFF: none)}
 * Refused before any HIP call: n above 2^20, max_steps outside 1..32 or n * max_steps above 2^22, a projection outside the context (-1);
 * an input that is not a number, an energy outside the cross-section tables, a direction of length zero (-2). */
#define MCGPU_KAT_LOOKUP 0
#define MCGPU_KAT_FLIGHT 1
int mcgpu_kat_flight(mcgpu_ctx *ctx, int mode, int kind, int projection, int n, int max_steps, unsigned int seed, const float *in8,
                     const unsigned long long *in_u64, uint32_t *out_u32);
/* The 16-byte record of a 4x4x4 tile of a u8-palette volume as the host and the device build it (csrc/device_model.hpp:
 * encode_tile_record; no reference counterpart -- the reference gathers the voxel itself, MC-GPU_kernel_v1.3.cu:262-266).  Host code
 * only, no context: indices[t * 64 + v] = palette index of voxel v = (iz & 3) 16 + (iy & 3) 4 + (ix & 3) of tile t, negative = padding
 * of an edge tile; out_u32[t * 4 ..] = {entries a | b << 8 | c << 16 | d << 24, code, mask low, mask high}. */
int mcgpu_kat_tile_records(int n_tiles, const short *indices, uint32_t *out_u32);

/* ------------------------------------------------------------------------------------------------
 * Row f4: FDK reconstruction of a projection stack (what the reference obtains from `rtkfdk --hardware cuda`,
 * cbctmc/reconstruction/reconstruction.py:22-69).  RTK geometry conventions (rotation axis y, source at
 * Ry(gantry) (0,0,sid), detector coordinate u = sdd x'/(sid - z') - proj_offset_x); projections are line integrals
 * [n_proj][nv][nu] on the host, pixel (i, j) centred at (u0 + i du, v0 + j dv); the volume is written [nz][ny][nx],
 * voxel (0,0,0) centred at (ox, oy, oz) (NaN = volume centred on the isocentre).  hann / hann_y: cut-off of the Hann
 * windows as fractions of Nyquist (0 = plain ramp / no vertical smoothing); wpc: optional water pre-correction
 * polynomial coefficients (rtkfdk --wpc).  Displaced (half-fan) detectors are weighted automatically. */
typedef struct mcgpu_fdk_options {
  unsigned int struct_size;     /* sizeof(mcgpu_fdk_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int n_proj, nu, nv;
  double du, dv, u0, v0;
  double sid, sdd;
  const double *gantry_deg;     /* [n_proj] */
  const double *proj_offset_x;  /* [n_proj] or NULL (0) */
  const double *proj_offset_y;  /* [n_proj] or NULL (0) */
  int nx, ny, nz;
  double sx, sy, sz, ox, oy, oz;
  double hann, hann_y;
  const double *wpc;
  int n_wpc;
  int device;
  double pad;                   /* rtkfdk --pad (truncation correction; the reference passes 1.0, reconstruction.py:29,55): rows
                                   continued on both sides by ceil(pad x width) columns, feathered point reflection; 0 = off.
                                   Follows the PUBLISHED heuristic (Ohnesorge et al.) as RTK describes it; the exact extent and
                                   weight table of rtkFFTProjectionsConvolutionImageFilter could not be checked here (RTK is not
                                   vendored in the reference): with a truncated half-fan scan the feathered edge values fed to the
                                   ramp may differ from rtkfdk's ("parity unpinned") */
} mcgpu_fdk_options;
typedef struct mcgpu_fdk_report {
  double ms_filter;      /* weight + ramp + vertical smoothing kernels */
  double ms_backproject; /* back-projection kernels */
} mcgpu_fdk_report;
int mcgpu_fdk_reconstruct(const mcgpu_fdk_options *options, const float *projections, float *volume, mcgpu_fdk_report *report);

/* Row f15: motion-compensated FDK (Rit et al., Med. Phys. 36 (2009); what RTK's FDKWarpBackProjectionImageFilter does for
 * `rtkfdk --signal --dvf`; csrc/fdk.hip: backproject_motion_kernel, whose header states the rule).  The filter chain is that of
 * mcgpu_fdk_reconstruct; the back-projector takes the sample of projection i for the voxel at P at P + mean(P) + sum_k
 * coefficients[k](P) delta[i][k], the place where the model puts that voxel's material at the projection's breathing state.
 * mean [3][nz][ny][nx] and coefficients [K][3][nz][ny][nx] live on the reconstruction grid, in mm (mm per signal unit), components
 * along IEC X, Y, Z; delta[i][k] = signal_i[k] - mean_signal[k] (rounded once to float32).  The model maps the reference-phase
 * volume forward; a pull-back model is NOT inverted.  Parity against RTK's warp back-projector is unpinned (RTK is absent here). */
typedef struct mcgpu_fdk_motion {
  unsigned int struct_size;     /* sizeof(mcgpu_fdk_motion) as the caller was compiled; 0 is refused */
  int n_signal_dims;            /* K, 1..4 */
  const float *mean;            /* [3][nz][ny][nx] */
  const float *coefficients;    /* [K][3][nz][ny][nx] */
  const double *delta;          /* [n_proj][K], finite */
} mcgpu_fdk_motion;
typedef struct mcgpu_fdk_motion_report {
  double ms_filter;       /* as mcgpu_fdk_report */
  double ms_backproject;  /* the motion back-projection kernels */
  double ms_upload_model; /* host clock around the model's upload */
  unsigned long long peak_device_bytes;
} mcgpu_fdk_motion_report;
int mcgpu_fdk_reconstruct_motion(const mcgpu_fdk_options *options, const mcgpu_fdk_motion *motion, const float *projections, float *volume,
                                 mcgpu_fdk_motion_report *report);

/* ------------------------------------------------------------------------------------------------
 * Row f13: the normal equations of the empirical water pre-correction (Sourbelle et al. 2005; what the reference's
 * scripts/fit_wpc.py computes from N + 1 rtkfdk runs), fused on the device (csrc/wpc_fit.hip; the rule: DESIGN.md row f13).
 * With q the normalised projections of a water phantom, f_n = FDK(q^n) is what mcgpu_fdk_reconstruct gives for the wpc
 * polynomial e_n, n = 0..order.  The call forms the slab means fbar_n[z][x] = sum_{y in [y_first, y_first + y_count)} f_n[z][y][x]
 * / y_count (float32) without ever holding a volume, and B[i][j] = sum_pixels weight fbar_i fbar_j, a[i] = sum_pixels weight
 * fbar_i template in double, summed in a fixed order: two calls give the same bytes.  The coefficients c = inv(B) a are left to
 * the caller.  All fields but order, y_first, y_count and channel_layout mean what they mean in mcgpu_fdk_options. */
typedef struct mcgpu_wpc_fit_options {
  unsigned int struct_size;     /* sizeof(mcgpu_wpc_fit_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int n_proj, nu, nv;
  double du, dv, u0, v0;
  double sid, sdd;
  const double *gantry_deg;     /* [n_proj] */
  const double *proj_offset_x;  /* [n_proj] or NULL (0) */
  const double *proj_offset_y;  /* [n_proj] or NULL (0) */
  int nx, ny, nz;
  double sx, sy, sz, ox, oy, oz;
  double hann, hann_y, pad;
  int order;                    /* N, 1..7: the powers q^0 .. q^N */
  int y_first, y_count;         /* the slab of the volume's y axis: y_count >= 1, inside [0, ny) */
  int device;
  int channel_layout;           /* of the filtered powers the back-projector samples: 0 = the faster one as measured
                                   (profiles/wpc_fit_ab.md), 1 = one plane per power, 2 = the powers interleaved per pixel; the
                                   results are the same bit for bit */
} mcgpu_wpc_fit_options;
typedef struct mcgpu_wpc_fit_report {
  double ms_upload;             /* host -> device copies of the projections (wall time) */
  double ms_filter;             /* power-basis weighting, extension, ramp, hannY (and the interleaving pass) */
  double ms_backproject;        /* slab-mean back-projection kernels */
  double ms_reduce;             /* the normal-equation kernel */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once, hipFFT's work areas included */
} mcgpu_wpc_fit_report;
int mcgpu_wpc_fit(const mcgpu_wpc_fit_options *options, const float *projections /*[n_proj][nv][nu]*/, const float *weight /*[nz][nx]*/,
                  const float *template_ /*[nz][nx]*/, double *B /*[order + 1][order + 1]*/, double *a /*[order + 1]*/,
                  float *basis_mean /*[order + 1][nz][nx], may be NULL*/, mcgpu_wpc_fit_report *report);

/* ------------------------------------------------------------------------------------------------
 * Joseph forward projection on the circular cone-beam geometry of the FDK options above: what the reference obtains from RTK's
 * JosephForwardProjectionImageFilter, cbctmc/forward_projection.py: project_forward (csrc/forward_project.hip).  Output
 * [n_proj][nv][nu] line integrals (sum of density x mm), pixel (i, j) centred at (u0 + i du, v0 + j dv).  The volume
 * [nz][ny][nx] is in RTK's IEC frame, voxel (0,0,0) centred at (ox, oy, oz) (NaN = volume centred on the isocentre); it spans
 * half a voxel beyond its outer voxel centres and is 0 outside.  Parity against RTK's own border handling is unpinned. */
typedef struct mcgpu_fp_options {
  unsigned int struct_size;     /* sizeof(mcgpu_fp_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int n_proj, nu, nv;
  double du, dv, u0, v0;
  double sid, sdd;
  const double *gantry_deg;     /* [n_proj] */
  const double *proj_offset_x;  /* [n_proj] or NULL (0) */
  const double *proj_offset_y;  /* [n_proj] or NULL (0) */
  int nx, ny, nz;               /* mcgpu_forward_project_context: 0 = the context's size, else must equal it */
  double sx, sy, sz;            /* mm; mcgpu_forward_project_context: 0 = the context's voxel size */
  double ox, oy, oz;
  int device;                   /* mcgpu_forward_project only (a context projects on its own device) */
} mcgpu_fp_options;
typedef struct mcgpu_fp_report {
  double ms_kernel;  /* projection kernels */
  double ms_upload;  /* host -> device copy of the volume (0 for a context) */
} mcgpu_fp_report;
/* A float volume from the host; no context needed. */
int mcgpu_forward_project(const mcgpu_fp_options *options, const float *volume, float *projections, mcgpu_fp_report *report);
/* The context's current geometry (after mcgpu_set_geometry_arrays or mcgpu_warp_geometry), read in place on the device.  Its
 * volume is stored in the .vox frame (vox x, y, z = MC y, -MC x, MC z); IEC (X, Y, Z) = (-vox y, -vox z, -vox x), i.e. the
 * IEC size is (vox ny, vox nz, vox nx). */
int mcgpu_forward_project_context(mcgpu_ctx *ctx, const mcgpu_fp_options *options, float *projections, mcgpu_fp_report *report);

/* ------------------------------------------------------------------------------------------------
 * Row f17: the ray-traced primary (csrc/primary_project.hip, whose header states the rule).  The expectation of the `unscattered`
 * plane of projections first_projection .. + n_projections - 1 of the geometry, poses, detector and spectrum resident in the
 * context: source spectrum x Beer-Lambert attenuation along the line focal spot -> pixel through the context's voxels, with the
 * cross-section tables of the flight step.  planes: [n_projections][nz][crop_nx] float32 in finalize's layout and unit (eV / cm^2
 * per history, z flipped, the first crop_nx columns).  Refused with -1 before any device work: a context without a device, a
 * projection range outside the context's, su / sv outside 1..8, energy_points outside 1..4. */
typedef struct mcgpu_primary_options {
  unsigned int struct_size;  /* sizeof(mcgpu_primary_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int first_projection;
  int n_projections;         /* 0: one */
  int su, sv;                /* sub-points per pixel along x / z, 1..8 (0: 1) */
  int energy_points;         /* Gauss-Legendre points per spectrum bin, 1..4 (0: 2) */
  int crop_nx;               /* as mcgpu_finalize_projection: outside 1 .. nx - 1 = the full width */
} mcgpu_primary_options;
typedef struct mcgpu_primary_report {
  unsigned int struct_size;  /* sizeof(mcgpu_primary_report) as the caller was compiled: that many bytes are written */
  int n_materials;           /* materials of the device model (columns of the cross-section table) */
  double ms_kernel;          /* projection kernels */
  double ms_tables;          /* spectrum nodes, cross-sections, poses and the solid angle on the host, and their upload */
  double solid_angle;        /* of the source aperture [sr] */
  int n_energy_points;       /* spectrum nodes in all */
  int reserved;
  double ms_sample;          /* mcgpu_primary_noisy: the sampler's kernels (0 for the other calls) */
} mcgpu_primary_report;
int mcgpu_primary_project(mcgpu_ctx *ctx, const mcgpu_primary_options *options, float *planes, mcgpu_primary_report *report);
/* Row f20: the noise of the ray-traced primary (the header of csrc/primary_project.hip states the moment planes and THE NOISE RULE).
 * mcgpu_primary_moments: the planes M_0, M_1, M_2 of every projection -- photons / cm^2, eV / cm^2, eV^2 / cm^2 per history; M_1 is
 * mcgpu_primary_project's plane, bit for bit -- from one traversal: planes [n_projections][3][nz][crop_nx].  Same options, report
 * and refusals as mcgpu_primary_project. */
int mcgpu_primary_moments(mcgpu_ctx *ctx, const mcgpu_primary_options *options, float *planes, mcgpu_primary_report *report);
/* mcgpu_primary_noisy: the `unscattered` plane with the mean and the variance that `histories` histories of the engine would give
 * it: the moments and the compound Poisson sampler run on the device, only the sampled planes [n_projections][nz][crop_nx] come
 * back.  The pixel area is the context's detector's.  A function of (seed, first_projection + p, pixel): the same seed gives the
 * same bytes, and a scan made in two calls equals one call.  Refused as mcgpu_primary_project refuses, and histories <= 0 or not
 * finite. */
typedef struct mcgpu_primary_noisy_options {
  unsigned int struct_size;  /* sizeof(mcgpu_primary_noisy_options) as the caller was compiled; 0 is refused */
  int first_projection;
  int n_projections;         /* 0: one */
  int su, sv;                /* as mcgpu_primary_options */
  int energy_points;
  int crop_nx;
  int reserved;
  double histories;          /* N > 0: the history count whose noise the plane carries (need not be whole) */
  unsigned long long seed;   /* key of the Philox4x32-10 draws */
} mcgpu_primary_noisy_options;
int mcgpu_primary_noisy(mcgpu_ctx *ctx, const mcgpu_primary_noisy_options *options, float *planes, mcgpu_primary_report *report);
/* The sampler alone, on host planes [n_planes][ny][nx] of `device`: THE NOISE RULE with the moments m0, m1, m2, N = histories and
 * a = pixel_area [cm^2]; plane p draws with counter (x, y, first_projection + p, k).  Refused with -1 before any device call: a
 * null plane, n_planes outside 1 .. 65535, ny or nx < 1, ny x nx of 2^31 and more, first_projection < 0, histories or pixel_area
 * not finite or <= 0. */
int mcgpu_sample_compound_poisson(int device, const float *m0, const float *m1, const float *m2, float *out, int n_planes, int ny, int nx,
                                  double histories, double pixel_area, unsigned long long seed, int first_projection);
/* out = max(0, mean + sqrt(max(variance, 0)) z2), z2 the normal of draw k = 2 at counter (x, y, first_projection + p, 2): the noise
 * of a smoothed scatter plane.  Same shapes and refusals as mcgpu_sample_compound_poisson. */
int mcgpu_sample_gaussian(int device, const float *mean, const float *variance, float *out, int n_planes, int ny, int nx,
                          unsigned long long seed, int first_projection);
/* scipy.ndimage.gaussian_filter(plane, (sigma_y, sigma_x), truncate = 4, mode = "reflect") of n_planes float32 planes [ny][nx] on
 * `device` (host pointers; planes_out may be planes_in).  A sigma of 0 skips its axis; both 0 copy the planes bit for bit without
 * touching the device.  ms_kernel (may be NULL): the passes' device time. */
int mcgpu_smooth_planes(int device, const float *planes_in, float *planes_out, int n_planes, int ny, int nx, double sigma_y, double sigma_x,
                        double *ms_kernel);

/* ------------------------------------------------------------------------------------------------
 * Row f6: 4-D ROOSTER reconstruction (what the reference obtains from RTK's `rtkfourdrooster`,
 * cbctmc/reconstruction/reconstruction.py: reconstruct_4d; csrc/rooster4d.hip, whose header spells out the algorithm).
 * Geometry, detector grid, volume grid and wpc as mcgpu_fdk_options; the result is n_frames volumes [n_frames][nz][ny][nx]
 * of the FDK grid.  phase[k] in [0, 1] places projection k between frames floor(phase N) mod N and the next one (periodic).
 * Each of niter main iterations runs cgiter conjugate-gradient steps on S^T B R S x = S^T B p (R = Joseph forward projection,
 * B = its approximate adjoint, S = the phase interpolation), then positivity (when `positivity` is non-zero), then tviter
 * iterations of spatial TV denoising (gamma_space) of every frame and of temporal TV denoising (gamma_time, periodic) of every
 * voxel's series.  Parity against rtkfourdrooster itself is unpinned (RTK is absent here). */
typedef struct mcgpu_rooster4d_options {
  unsigned int struct_size;     /* sizeof(mcgpu_rooster4d_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int n_proj, nu, nv;           /* nu, nv >= 2 */
  double du, dv, u0, v0;
  double sid, sdd;
  const double *gantry_deg;     /* [n_proj] */
  const double *proj_offset_x;  /* [n_proj] or NULL (0) */
  const double *proj_offset_y;  /* [n_proj] or NULL (0) */
  int nx, ny, nz;
  double sx, sy, sz, ox, oy, oz; /* mm; origin = centre of voxel (0,0,0), NaN = volume centred on the isocentre */
  int n_frames;                 /* 1..32 */
  const double *phase;          /* [n_proj], each in [0, 1] */
  int niter, cgiter, tviter;
  double gamma_space, gamma_time;
  int positivity;               /* non-zero: x = max(x, 0) after the CG steps of every main iteration */
  const double *wpc;            /* water pre-correction polynomial (rtkfdk --wpc) applied to the projections, or NULL */
  int n_wpc;
  int device;
  double *residuals;            /* optional [niter][cgiter + 1]: |r| at the restart and after each CG step of every main iteration */
} mcgpu_rooster4d_options;
typedef struct mcgpu_rooster4d_report {
  double ms_forward;            /* R S: 4-D forward projection kernels */
  double ms_back;               /* S^T B: 4-D back-projection kernels */
  double ms_cg_vectors;         /* CG vector updates, dot products, positivity */
  double ms_tv_space;           /* spatial TV kernels */
  double ms_tv_time;            /* temporal TV kernel */
  double ms_upload;             /* host -> device copies (and the water pre-correction) */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once */
} mcgpu_rooster4d_report;
int mcgpu_rooster4d_reconstruct(const mcgpu_rooster4d_options *options, const float *projections /*[n_proj][nv][nu]*/,
                                float *volume4d /*[n_frames][nz][ny][nx]*/, mcgpu_rooster4d_report *report);
/* One operator alone (for tests): FORWARD in = 4-D volume -> out = projections (R S); BACK in = projections -> out = 4-D volume
 * (S^T B; no water pre-correction); TV_SPACE / TV_TIME in = 4-D volume -> out = 4-D volume (tviter iterations, gamma_space /
 * gamma_time).  niter, cgiter, positivity and residuals are not used. */
enum { MCGPU_ROOSTER4D_STAGE_FORWARD = 0, MCGPU_ROOSTER4D_STAGE_BACK = 1, MCGPU_ROOSTER4D_STAGE_TV_SPACE = 2, MCGPU_ROOSTER4D_STAGE_TV_TIME = 3 };
int mcgpu_rooster4d_stage(const mcgpu_rooster4d_options *options, int stage, const float *in, float *out, mcgpu_rooster4d_report *report);

/* Row f16: motion-aware 4-D ROOSTER (Mory, Janssens, Rit, PMB 2016; what RTK's `rtkfourdrooster --dvf --idvf` is for;
 * csrc/rooster4d.hip, whose header states the rule).  Row f6 with its temporal TV run along the trajectories of two linear motion
 * models on the reconstruction grid, both in the layout of row f15: mean [3][nz][ny][nx] and coefficients [K][3][nz][ny][nx], mm
 * (mm per signal unit) along IEC X, Y, Z, the same K for both.
 *   to_reference   (forward model): the material of reference-phase voxel P is at P + F(P; s) at state s;
 *   from_reference (pull-back model): frame_s(Q) = ref(Q + G(Q; s)).
 * Frame f has a state s_f; delta_to[f][k] = s_f[k] - mean_signal_to[k], delta_from[f][k] likewise (rounded once to float32).
 * The sampling operator Sigma(model, delta) of a volume at voxel (ix, iy, iz): displacement d = mean + sum_k coefficients[k]
 * delta[k] (fmaf chain, k ascending); per axis fx = fmaf(d_x, 1 / sx, (float)ix) clamped to [0, nx - 1] by fminf(fmaxf(fx, 0),
 * nx - 1) (the border is replicated; every index is in bounds for any float input), i0 = (int)floorf(fx), t = fx - i0, i1 =
 * min(i0 + 1, nx - 1); trilinear with nested lerp(a, b, t) = fmaf(t, b - a, a) along x, y, z.  W applies Sigma(to_reference,
 * delta_to[f]) to frame f, U applies Sigma(from_reference, delta_from[f]).  Steps 1 - 3 of a main iteration are those of row f6;
 * step 4 is  y = W x;  c = TVtime(y) - y;  x = x + U c  (the increment form: only the correction is resampled; RTK replaces x by
 * U TVtime(W x)).  With gamma_time = 0 or tviter = 0 step 4 leaves x untouched.  No model is derived from the other and a swapped
 * pair is not detected.  Parity against RTK is unpinned (RTK is absent here). */
typedef struct mcgpu_rooster4d_motion {
  unsigned int struct_size;     /* sizeof(mcgpu_rooster4d_motion) as the caller was compiled; 0 is refused */
  int n_signal_dims;            /* K, 1..4 */
  const float *to_reference_mean;            /* [3][nz][ny][nx] */
  const float *to_reference_coefficients;    /* [K][3][nz][ny][nx] */
  const float *from_reference_mean;          /* [3][nz][ny][nx] */
  const float *from_reference_coefficients;  /* [K][3][nz][ny][nx] */
  const double *delta_to;       /* [n_frames][K], finite */
  const double *delta_from;     /* [n_frames][K], finite */
} mcgpu_rooster4d_motion;
typedef struct mcgpu_rooster4d_motion_report {
  double ms_forward, ms_back, ms_cg_vectors, ms_tv_space, ms_tv_time, ms_upload, ms_total;  /* as mcgpu_rooster4d_report */
  unsigned long long peak_device_bytes;
  double ms_warp;               /* the W and U kernels and the subtraction between them */
  double ms_upload_model;       /* host clock around the upload of the two models */
} mcgpu_rooster4d_motion_report;
/* Refused with -1 before any device call: what mcgpu_rooster4d_reconstruct refuses, a null model or delta pointer, K outside 1..4,
 * a delta that is not finite (as float32), an unknown stage. */
int mcgpu_rooster4d_reconstruct_motion(const mcgpu_rooster4d_options *options, const mcgpu_rooster4d_motion *motion,
                                       const float *projections /*[n_proj][nv][nu]*/, float *volume4d /*[n_frames][nz][ny][nx]*/,
                                       mcgpu_rooster4d_motion_report *report);
/* One operator alone (for tests), 4-D volume -> 4-D volume: WARP out = W in; UNWARP out = U in; TV_TIME_MOTION out = in +
 * U (TVtime(W in) - W in) with tviter iterations and gamma_time.  The geometry fields of the options are checked and not used. */
enum { MCGPU_ROOSTER4D_MOTION_STAGE_WARP = 0, MCGPU_ROOSTER4D_MOTION_STAGE_UNWARP = 1, MCGPU_ROOSTER4D_MOTION_STAGE_TV_TIME_MOTION = 2 };
int mcgpu_rooster4d_motion_stage(const mcgpu_rooster4d_options *options, const mcgpu_rooster4d_motion *motion, int stage, const float *in,
                                 float *out, mcgpu_rooster4d_motion_report *report);

/* ------------------------------------------------------------------------------------------------
 * Row f14: demons registration of two volumes (what the reference's CorrespondenceModel.build_default obtains from vroc's
 * variational registration, cbctmc/registration/correspondence.py:315-345; csrc/registration.hip, whose header states the rule;
 * float64 restatement: tests/registration_ref.py).  fixed, moving and the mask are [nx][ny][nz] (nz fastest in memory: the arrays
 * of an MCGeometry and of CorrespondenceModel.fit(frame="geometry")); the result is a displacement field [3][nx][ny][nz] in
 * voxels on the fixed grid with moving(x + u(x)) ~ fixed(x), component i along array axis i: what mcgpu_warp_geometry(frame 1)
 * and mcgpu_correspondence_fit take.  Every kernel is a fixed function of its inputs: two calls give the same bytes.  Parity
 * against vroc itself is unpinned (vroc is absent here). */
enum { MCGPU_REGISTER_MAX_LEVELS = 8 };
typedef struct mcgpu_register_options {
  unsigned int struct_size;     /* sizeof(mcgpu_register_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int nx, ny, nz;               /* the volumes' shape; fewer than 2^31 voxels */
  int iterations;               /* per level, >= 0; no early stop */
  int n_levels;                 /* 1..MCGPU_REGISTER_MAX_LEVELS: level l = n_levels - 1 .. 0 has shape ceil(n / 2^l) */
  int device;
  int out_nx, out_ny, out_nz;   /* mcgpu_register_stage, the two resize stages only: the shape of `out` */
  double tau;                   /* step width */
  double sigma[3];              /* of the Gaussian that smooths the field after every step, in voxels per axis: 0 skips the axis's
                                   pass, more than 4 is refused (radius int(4 sigma + 0.5) <= 16) */
  float *differences;           /* optional: for every level, coarsest first, warped moving - fixed of the level [sx][sy][sz] before
                                   its first iteration and then after its last: what the report's mean squares are the means of */
} mcgpu_register_options;
typedef struct mcgpu_register_report {
  unsigned int struct_size;     /* sizeof(mcgpu_register_report) as the caller was compiled; only that many bytes are written */
  int n_levels;
  double msd_before[MCGPU_REGISTER_MAX_LEVELS];  /* [l]: mean over the level's voxels of double(float32(warped moving - fixed))^2 */
  double msd_after[MCGPU_REGISTER_MAX_LEVELS];   /* before the first and after the last iteration of level l (0 = finest); summed in double in a fixed order */
  double ms_upload;             /* host <-> device copies (wall time) */
  double ms_resize;             /* images, mask and field to a level's shape */
  double ms_force;              /* steps 1 to 5: warp, difference, gradient, update */
  double ms_smooth;             /* the Gaussian passes */
  double ms_reduce;             /* the mean squared differences */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once */
} mcgpu_register_report;
int mcgpu_register(const mcgpu_register_options *options, const float *fixed, const float *moving, const unsigned char *fixed_mask_or_null,
                   float *field_out /*[3][nx][ny][nz]*/, mcgpu_register_report *report);
/* One operator alone (for tests).  RESIZE_LINEAR: moving [nx][ny][nz] -> out float [out_nx][out_ny][out_nz]; RESIZE_NEAREST:
 * fixed_mask -> out uint8 of that shape; WARP_LINEAR: moving, field -> out float [nx][ny][nz] = moving(x + u); FORCE_STEP: fixed,
 * moving, field, fixed_mask (or NULL) -> out [3][nx][ny][nz] = u + tau v; SMOOTH: field -> out [3][nx][ny][nz].  Arguments a
 * stage does not read may be NULL; iterations, n_levels and differences are not used. */
enum { MCGPU_REGISTER_STAGE_RESIZE_LINEAR = 0, MCGPU_REGISTER_STAGE_RESIZE_NEAREST = 1, MCGPU_REGISTER_STAGE_WARP_LINEAR = 2,
       MCGPU_REGISTER_STAGE_FORCE_STEP = 3, MCGPU_REGISTER_STAGE_SMOOTH = 4 };
int mcgpu_register_stage(const mcgpu_register_options *options, int stage, const float *fixed, const float *moving, const float *field,
                         const unsigned char *fixed_mask_or_null, void *out, mcgpu_register_report *report);

/* ------------------------------------------------------------------------------------------------
 * Row f22: the inverse of a displacement field by fixed-point iteration, and the residual of a pair of fields
 * (csrc/field_inverse.hip, whose header states the rule; float64 restatement: tests/field_inverse_ref.py).  Fields are
 * [3][nx][ny][nz] float32 in voxels, component i along array axis i, nz fastest in memory: mcgpu_register's result.  The inverse v
 * of u satisfies u(x + v(x)) + v(x) ~ 0: if moving(x + u(x)) ~ fixed(x) then fixed(y + v(y)) ~ moving(y).  One step is
 * v <- v - relaxation r with the residual r(x) = v(x) + u(x + v(x)) (u sampled as mcgpu_register samples the moving image:
 * trilinear, coordinates clamped), Jacobi, no early stop: the result is a function of (u, initial, iterations, relaxation), two
 * calls give the same bytes.  The fields must be finite (not checked here; the Python layer refuses others).
 * Refused with -1 before any device call: struct_size 0, a null pointer, a size below 1, 2^31 voxels or more, negative iterations,
 * a relaxation that is not finite or outside (0, 1], a negative device. */
typedef struct mcgpu_invert_options {
  unsigned int struct_size;     /* sizeof(mcgpu_invert_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int nx, ny, nz;               /* the fields' shape; fewer than 2^31 voxels */
  int iterations;               /* steps, >= 0; mcgpu_field_residual takes none */
  int device;
  double relaxation;            /* 0 < relaxation <= 1, rounded to float32; 1 converges only where the finite differences of u stay
                                   below 1, 0.5 takes differences up to 3 */
  const float *initial;         /* v_0 [3][nx][ny][nz], or NULL for zeros; mcgpu_field_residual does not read it */
} mcgpu_invert_options;
typedef struct mcgpu_invert_report {
  unsigned int struct_size;     /* sizeof(mcgpu_invert_report) as the caller was compiled; only that many bytes are written */
  int iterations;               /* the steps that were taken */
  double residual_max_before;   /* max over components and voxels of |r_i(x)| before the first step */
  double residual_rms_before;   /* sqrt(sum double(r_i)^2 / (3 N)), summed in double in a fixed order */
  double residual_max_after;    /* the same two after the last step (mcgpu_field_residual leaves them 0) */
  double residual_rms_after;
  double ms_upload;             /* host <-> device copies (wall time) */
  double ms_step;               /* the steps */
  double ms_reduce;             /* the residuals */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once: 9 N floats and the partial sums */
} mcgpu_invert_report;
int mcgpu_invert_field(const mcgpu_invert_options *options, const float *field /*[3][nx][ny][nz]*/, float *inverse_out /*[3][nx][ny][nz]*/,
                       mcgpu_invert_report *report);
/* r(x) = v(x) + u(x + v(x)) of two fields, no steps: fills residual_max_before and residual_rms_before, and residual_out where
 * that is given.  About zero where v is the inverse of u; about 2 |u| where v = u. */
int mcgpu_field_residual(const mcgpu_invert_options *options, const float *u, const float *v, float *residual_out_or_null /*[3][nx][ny][nz]*/,
                         mcgpu_invert_report *report);

/* ------------------------------------------------------------------------------------------------
 * Row f21: the breathing signal from the projections alone (what RTK does with rtkamsterdamshroud followed by
 * rtkextractshroudsignal; csrc/shroud.hip, whose header states the rule; float64 restatement: tests/shroud_ref.py).  Stage A forms
 * the Amsterdam shroud A[n_proj][m] (float32) from the projections, stage B the costs c_i(s) of shifting column i against column
 * i - 1 by s rows, stage C the signal x[n_proj] in rows (x_0 = 0; positive: toward larger v).  Every kernel is a fixed function of
 * its inputs: two calls give the same bytes.  The amplitude is not calibrated: the signal serves for the phase.  Parity against RTK
 * itself is unpinned (RTK is absent here). */
typedef struct mcgpu_shroud_options {
  unsigned int struct_size;     /* sizeof(mcgpu_shroud_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int n_proj, nu, nv;           /* the stack [n_proj][nv][nu]; mcgpu_shroud_signal: n_proj columns */
  int u_first, u_count;         /* the columns that are summed; u_count 0: all columns from u_first on */
  int v_first, v_count;         /* the rows that make the shroud, m = v_count; v_count 0: all rows from v_first on */
  int unsharp;                  /* width of the unsharp mask along the projection axis: odd, or 0 for none; an even one is refused */
  int max_shift;                /* S: shifts -S .. S rows are tried; 2 S < m is required */
  int device;
} mcgpu_shroud_options;
typedef struct mcgpu_shroud_report {
  unsigned int struct_size;     /* sizeof(mcgpu_shroud_report) as the caller was compiled; only that many bytes are written */
  int reserved;
  double ms_upload;             /* host -> device copies (wall time) */
  double ms_shroud;             /* stage A: row sums, their combination, the unsharp mask */
  double ms_cost;               /* stage B */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once: the stack goes up 32 projections at a time */
} mcgpu_shroud_report;
/* Stages A to C.  Refused with -1 before any device call: a size below 1, columns or rows outside the image, an even unsharp, a
 * negative max_shift or 2 max_shift >= m, a null projections or signal pointer. */
int mcgpu_shroud_extract(const mcgpu_shroud_options *options, const float *projections /*[n_proj][nv][nu]*/, float *shroud /*[n_proj][m] or NULL*/,
                         double *costs /*[n_proj - 1][2 S + 1] or NULL*/, double *signal /*[n_proj]*/, mcgpu_shroud_report *report);
/* Stages B and C alone from a shroud on the host (for tests with crafted columns): n_proj and v_count give its shape and max_shift
 * gives S; nu, nv, u_first, u_count, v_first and unsharp are not read. */
int mcgpu_shroud_signal(const mcgpu_shroud_options *options, const float *shroud /*[n_proj][v_count]*/, double *costs /*[n_proj - 1][2 S + 1] or NULL*/,
                        double *signal /*[n_proj]*/, mcgpu_shroud_report *report);
/* The row sums D[n_proj][m] (float64, before the mask) of a stack that is resident on options->device, written to device memory:
 * what tools/shroud_bench.py times.  unsharp and max_shift are not used; the call returns when the kernels have finished. */
int mcgpu_shroud_rows_device(const mcgpu_shroud_options *options, const float *projections_device, double *rows_device /*[n_proj][m]*/,
                             mcgpu_shroud_report *report);

/* ------------------------------------------------------------------------------------------------
 * The speed-up network (what the reference obtains from cbctmc/speedup/inference.py: MCSpeedup; csrc/speedup_net.hip, whose
 * header restates the network).  Two U-Nets of 3 x 3 convolutions (replicate padding, bias), instance norm and LeakyReLU(0.01),
 * in float32: the mean net sees the low-photon projection and the forward projection (matched to it in mean and unbiased
 * std per projection), the variance net sees the mean.  mean = relu(low_photon + 10 tanh(mean_net)), variance = mean x 0.10
 * sigmoid(var_net(mean)) + 1e-6, sample = mean + sqrt(variance) z.  z is standard normal by Box-Muller from Philox4x32-10 with
 * key (seed low, seed high) and counter (x, y, first_projection + p, 0): u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24,
 * z = sqrt(-2 ln u1) cos(2 pi u2).  Projections are independent: the result does not depend on how a stack is split into calls.
 * `weights` is one flat float32 buffer: for the mean net, then the variance net, the tensors init_conv, final_conv, enc_0 ..
 * enc_{L-1} (first, second convolution), dec_{L-1} .. dec_0 (first, second), each as weight [c_out][c_in][3][3] then bias
 * [c_out] (the order of the reference's state dict without var_scale; tests/golden/speedup_state_dict.json).
 * Refused before any device call (-1, mcgpu_last_error): a null input, an n_weights that is not the architecture's, nu or nv
 * not divisible by 2^levels of the deeper net, a net whose bottleneck would have fewer than 2 pixels, and a forward-projection
 * slice of zero variance (the reference divides by zero there and returns NaN). */
typedef struct mcgpu_speedup_options {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int device;
  int n, nu, nv;                /* stacks are [n][nv][nu] */
  int mean_in_channels;         /* 2: low photon + forward projection; 1: low photon alone (forward_projection must then be NULL) */
  int mean_levels, mean_filter_base;   /* the reference's: 4, 64 */
  int var_in_channels;          /* 1 */
  int var_levels, var_filter_base;     /* the reference's: 2, 16 */
  const float *weights;
  unsigned long long n_weights; /* 13,401,586 for the reference's architecture */
  unsigned long long seed;
  int first_projection;         /* projection index of slice 0 in the sampler's counter */
} mcgpu_speedup_options;
typedef struct mcgpu_speedup_report {
  double ms_upload;             /* host <-> device copies and the repacking of the weights */
  double ms_preprocess;         /* statistics and matching of the forward projection */
  double ms_conv;               /* convolution kernels */
  double ms_norm;               /* instance norm + LeakyReLU kernels */
  double ms_other;              /* max-pool, head, sampler */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once */
} mcgpu_speedup_report;
/* All stacks are host pointers to [n][nv][nu] float32; any of mean, variance, sample may be NULL. */
int mcgpu_speedup_run(const mcgpu_speedup_options *options, const float *low_photon, const float *forward_projection, float *mean,
                      float *variance, float *sample, mcgpu_speedup_report *report);
/* One operator alone (for tests), on images of nv rows x nu columns; the options' architecture, weights and n_weights are not
 * used.  CONV: in [c1][nv][nu] and optionally in2 [c2][nv2][nu2] (concatenated after in; with `upsample` in2 is read through the
 * x 2 nearest upsample and has nv2 = (nv + 1) / 2 rows and nu2 = (nu + 1) / 2 columns, else the size of in), weight
 * [c_out][c1 + c2][3][3], bias [c_out] -> out [c_out][nv][nu].  NORM_LRELU: in [c1][nv][nu] -> out.  MAXPOOL: in [c1][nv][nu] ->
 * out [c1][nv / 2][nu / 2].  PREPROCESS: in = low photon [n][nv][nu], in2 = forward projection -> out = the matched forward
 * projection.  NORMALS: out = z [n][nv][nu] of the options' seed and first_projection. */
enum { MCGPU_SPEEDUP_STAGE_CONV = 0, MCGPU_SPEEDUP_STAGE_NORM_LRELU = 1, MCGPU_SPEEDUP_STAGE_MAXPOOL = 2, MCGPU_SPEEDUP_STAGE_PREPROCESS = 3,
       MCGPU_SPEEDUP_STAGE_NORMALS = 4 };
typedef struct mcgpu_speedup_stage_args {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_stage_args); 0 is refused */
  int upsample;
  int c1, c2, c_out;
  const float *in, *in2, *weight, *bias;
  float *out;
} mcgpu_speedup_stage_args;
int mcgpu_speedup_stage(const mcgpu_speedup_options *options, int stage, const mcgpu_speedup_stage_args *args, mcgpu_speedup_report *report);

/* ------------------------------------------------------------------------------------------------
 * Training of the speed-up network on the device (what the reference obtains from cbctmc/speedup/trainer.py: MCSpeedUpTrainer;
 * csrc/speedup_train.hip, whose header states the rule).  A trainer is a handle: the flat weights (the order of
 * mcgpu_speedup_options.weights), both Adam moments, both packings of the weights and every buffer of a pass stay on the device
 * between steps.  A batch is n <= max_batch samples (low_photon, forward_projection or NULL, high_photon), host pointers to
 * [n][nv][nu] float32.  The forward pass is mcgpu_speedup_run's; the losses are means over n nv nu elements.
 *   phase MEAN:      loss = mean |m - t|; only the mean net's weights get gradients and move.
 *   phase VARIANCE:  loss = mean 0.5 (log v' + (m - t)^2 / v'), v' = max(v, 1e-6); the mean net is frozen, no gradient is taken
 *                    through m; only the variance net's weights get gradients and move.
 * Everything is float32 (no reduced-precision pass, no gradient scaling).  The batch gradient is the sum of the per-sample
 * gradients in sample order; nothing is accumulated atomically: the same call gives the same bytes.  The bias of a convolution
 * that feeds an instance norm has gradient exactly 0 by definition here (mathematically it is 0) and never
 * moves.  Adam: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2, w <- w - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + 1e-8), no
 * weight decay; t counts the updates of the phase's net; lr <- lr gamma after every update.
 * Refused before any device call (-1, mcgpu_last_error): a null handle or array, an unknown phase, n outside 1..max_batch, a
 * forward projection given to (or missing from) the architecture, a forward-projection slice of zero variance; by
 * mcgpu_speedup_train_create: a bad architecture, n_weights that is not the architecture's, nu or nv not divisible by 2^levels of
 * the deeper net, a bottleneck of fewer than 2 pixels, lr, gamma or betas out of range.
 * With `dry` set the handle is a plan: nothing touches the device, mcgpu_speedup_train_get_state reports planned_device_bytes,
 * and calls that would run refuse after their other checks. */
typedef struct mcgpu_speedup_trainer mcgpu_speedup_trainer;
enum { MCGPU_SPEEDUP_PHASE_MEAN = 0, MCGPU_SPEEDUP_PHASE_VARIANCE = 1 };
typedef struct mcgpu_speedup_train_options {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_train_options); 0 is refused */
  int device;
  int nu, nv, max_batch;        /* samples are [nv][nu]; the largest n of a later call */
  int mean_in_channels, mean_levels, mean_filter_base;   /* as mcgpu_speedup_options */
  int var_in_channels, var_levels, var_filter_base;
  int dry;                      /* 1: plan only */
  const float *weights;         /* the initial flat weights */
  unsigned long long n_weights;
  double lr, gamma;             /* the reference's: 1e-3, 0.99999 */
  double beta1, beta2;          /* 0.9, 0.999 */
} mcgpu_speedup_train_options;
typedef struct mcgpu_speedup_train_report {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_train_report) as the caller was compiled */
  int phase;
  double loss;                  /* the phase's: l1_loss or gaussian_nll_loss */
  double l1_loss, gaussian_nll_loss;
  double psnr_before, psnr_after;  /* 20 log10(8.711442 / sqrt(mse)) of low_photon and of the mean against high_photon */
  unsigned long long step;      /* updates done so far, both phases */
  double lr;                    /* the learning rate the next update will use */
  double ms_forward;            /* the copies of each sample to the device (they wait for it), preprocessing, both nets, heads, loss sums */
  double ms_wgrad;              /* weight- and bias-gradient kernels */
  double ms_dgrad;              /* input-gradient kernels, their fold, max-pool backward */
  double ms_norm;               /* backward of instance norm + LeakyReLU */
  double ms_optimizer;          /* Adam and the repacking of the weights */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the trainer has held */
} mcgpu_speedup_train_report;
typedef struct mcgpu_speedup_train_state {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_train_state); 0 is refused */
  int reserved;
  float *weights, *moment1, *moment2;  /* host, [n_weights] each; a NULL array is not transferred */
  unsigned long long n_weights;
  unsigned long long step_mean, step_variance;  /* updates of each net: Adam's t */
  double lr;
  unsigned long long planned_device_bytes;      /* get: what the trainer holds (a dry handle: would hold) */
} mcgpu_speedup_train_state;
int mcgpu_speedup_train_create(const mcgpu_speedup_train_options *options, mcgpu_speedup_trainer **handle);
/* One batch.  update = 1: gradient of the phase's loss, one Adam update, both packings redone; update = 0: the losses alone
 * (the reference's validate_on_batch), nothing changes. */
int mcgpu_speedup_train_step(mcgpu_speedup_trainer *handle, int phase, int n, const float *low_photon, const float *forward_projection,
                             const float *high_photon, int update, mcgpu_speedup_train_report *report);
/* The batch gradient of the phase's loss, [n_weights] in the order of the flat weights (zero outside the phase's net); changes
 * nothing. */
int mcgpu_speedup_train_gradients(mcgpu_speedup_trainer *handle, int phase, int n, const float *low_photon, const float *forward_projection,
                                  const float *high_photon, float *flat_gradient, mcgpu_speedup_train_report *report);
/* mean and variance [n][nv][nu] of the trainer's forward pass with its present weights (either may be NULL); changes nothing */
int mcgpu_speedup_train_predict(mcgpu_speedup_trainer *handle, int n, const float *low_photon, const float *forward_projection, float *mean,
                                float *variance);
/* Weights, moments, step counts and learning rate, device -> host and back: a run resumed from them continues bit for bit.
 * set: n_weights must be the trainer's (unless all three arrays are NULL); step counts and lr are always taken. */
int mcgpu_speedup_train_get_state(mcgpu_speedup_trainer *handle, mcgpu_speedup_train_state *state);
int mcgpu_speedup_train_set_state(mcgpu_speedup_trainer *handle, const mcgpu_speedup_train_state *state);
int mcgpu_speedup_train_destroy(mcgpu_speedup_trainer *handle);
/* One backward operator alone (for tests), on images of nv rows x nu columns; all arrays are host float32.
 *   CONV_WGRAD: in [c1][nv][nu], in2 [c2][nv2][nu2] or NULL (as MCGPU_SPEEDUP_STAGE_CONV, `upsample` included), in3 = dY
 *     [c_out][nv][nu] -> out = dW [c_out][c1 + c2][3][3], out2 = db [c_out] (may be NULL); values[0] = number of partials.
 *   CONV_DGRAD: in = dY [c_out][nv][nu], in2 = weight [c_out][c1 + c2][3][3] -> out = d in [c1][nv][nu], out2 = d in2
 *     [c2][nv2][nu2] (c2 > 0).
 *   NORM_LRELU_BACKWARD: in = x [c1][nv][nu] (before the norm), in2 = dy -> out = dx.
 *   MAXPOOL_BACKWARD: in = x [c1][nv][nu], in2 = dy [c1][nv / 2][nu / 2] -> out = dx.
 *   LOSS_L1: in = low_photon, in2 = the mean net's output, in3 = high_photon, each [n][nv][nu] -> out = dL/d(net output),
 *     out2 = mean (may be NULL), values[0] = loss.
 *   LOSS_NLL: in = mean, in2 = the variance net's output, in3 = high_photon -> out = dL/d(net output), out2 = variance (may be
 *     NULL), values[0] = loss.
 *   ADAM: in = gradient [n]; out = weights, out2 = moment 1, out3 = moment 2, each [n], updated in place by update number
 *     `step` (>= 1) with lr, beta1, beta2. */
enum { MCGPU_SPEEDUP_TRAIN_STAGE_CONV_WGRAD = 0, MCGPU_SPEEDUP_TRAIN_STAGE_CONV_DGRAD = 1, MCGPU_SPEEDUP_TRAIN_STAGE_NORM_LRELU_BACKWARD = 2,
       MCGPU_SPEEDUP_TRAIN_STAGE_MAXPOOL_BACKWARD = 3, MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_L1 = 4, MCGPU_SPEEDUP_TRAIN_STAGE_LOSS_NLL = 5,
       MCGPU_SPEEDUP_TRAIN_STAGE_ADAM = 6 };
typedef struct mcgpu_speedup_train_stage_args {
  unsigned int struct_size;     /* sizeof(mcgpu_speedup_train_stage_args); 0 is refused */
  int device;
  int nu, nv;
  int upsample, c1, c2, c_out;
  const float *in, *in2, *in3;
  float *out, *out2, *out3;
  double *values;               /* [4] or NULL */
  unsigned long long n;         /* losses: samples; ADAM: elements */
  unsigned long long step;
  double lr, beta1, beta2;
} mcgpu_speedup_train_stage_args;
int mcgpu_speedup_train_stage(int stage, const mcgpu_speedup_train_stage_args *args, mcgpu_speedup_train_report *report);

/* ------------------------------------------------------------------------------------------------
 * The CT segmentation network (what the reference obtains from cbctmc/segmentation/segmenter.py: MCSegmenter.segment;
 * csrc/segment_net.hip, whose header restates the network and the procedure).  A 3-D U-Net of 3 x 3 x 3 convolutions (zero
 * padding, bias), instance norm and LeakyReLU(0.01) in float32, run patch by patch; softmax over channels 0..7 and sigmoid on
 * channel 8 per patch, stitched as k + sum / n, then one-hot of the argmax (first maximum wins) and > 0.5.  The image is a host
 * array [shape[0]][shape[1]][shape[2]] (last axis fastest) of int16 or float32; it is rescaled [in_min, in_max] -> [out_min,
 * out_max] with clipping (not at all when the two ranges are equal) and padded with 0.0 up to the patch shape (left = pad / 2).
 * labels (uint8) and raw (float32, may be NULL) are [9][padded shape], padded = max(shape, patch_shape) per axis.
 * `weights` is one flat float32 buffer in the order of the reference's state dict: init_conv, final_conv, enc_0 .. enc_{L-1}
 * (first, second convolution), dec_{L-1} .. dec_0, each as weight [c_out][c_in][3][3][3] then bias [c_out]
 * (tests/golden/segment_state_dict.json).  n_filters = [init, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0, final], 2 levels + 2 values.
 * Refused before any device call (-1, mcgpu_last_error): a null pointer, a patch axis not divisible by 2^levels, a bottleneck of
 * fewer than 2 voxels, n_classes other than 9, a stride (1 - patch_overlap) x patch axis that is not a whole number >= 1,
 * filters or n_weights that do not fit together, and a footprint above memory_limit_bytes; a footprint above the device's free
 * memory is refused before anything is allocated. */
typedef struct mcgpu_segment_options {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_options) as the caller was compiled (later fields read as zero); 0 is refused */
  int device;
  int shape[3];                 /* the image */
  int image_type;               /* MCGPU_IMAGE_INT16 or MCGPU_IMAGE_FLOAT32 */
  int patch_shape[3];
  double patch_overlap;         /* stride = (1 - patch_overlap) x patch axis */
  int levels;                   /* 1..8; the reference's: 4 */
  int n_filters[18];            /* the reference's: 32 everywhere */
  int n_classes;                /* 9 */
  const float *weights;
  unsigned long long n_weights;
  double in_min, in_max;        /* the reference's: -1024, 3071 */
  double out_min, out_max;      /* the reference's: 0, 1; spans are taken in double and rounded to float32, as numpy does */
  unsigned long long memory_limit_bytes;  /* 0: the device's free memory alone decides */
} mcgpu_segment_options;
typedef struct mcgpu_segment_report {
  double ms_upload;             /* allocation, host <-> device copies and the repacking of the weights */
  double ms_conv;               /* convolution kernels */
  double ms_norm;               /* instance norm + LeakyReLU kernels */
  double ms_other;              /* patch staging, max-pool, head, stitching, mean and labels */
  double ms_total;              /* wall time of the call */
  unsigned long long patches_run;        /* distinct patch starts: each inferred once */
  unsigned long long patches_skipped;    /* repeats of a start that the rule gives: stitched again, not inferred again */
  unsigned long long peak_device_bytes;  /* most device memory the call held at once */
  unsigned long long planned_device_bytes;  /* what the call worked out before it allocated anything */
} mcgpu_segment_report;
int mcgpu_segment_run(const mcgpu_segment_options *options, const void *image, unsigned char *labels, float *raw, mcgpu_segment_report *report);
/* One operator alone (for tests), on tensors [c][shape[0]][shape[1]][shape[2]]; of the options only `device` is used.  CONV: in
 * [c1][shape] and optionally in2 [c2][shape2] (concatenated after in; with `upsample` in2 is read through the x 2 nearest upsample
 * and has (shape + 1) / 2 per axis, else shape), weight [c_out][c1 + c2][3][3][3], bias [c_out] -> out [c_out][shape].
 * NORM_LRELU: in [c1][shape] -> out.  MAXPOOL: in [c1][shape] -> out [c1][shape / 2].  HEAD: in = logits [9][shape] -> out.
 * STITCH: in = n_patches patches [c1][patch_shape] one after the other, starts [n_patches][3] in the volume `shape` -> out = mean
 * [c1][shape] (0 where no patch arrived).  FINALIZE: in = mean [9][shape] -> out = labels uint8 [9][shape]. */
enum { MCGPU_SEGMENT_STAGE_CONV = 0, MCGPU_SEGMENT_STAGE_NORM_LRELU = 1, MCGPU_SEGMENT_STAGE_MAXPOOL = 2, MCGPU_SEGMENT_STAGE_HEAD = 3,
       MCGPU_SEGMENT_STAGE_STITCH = 4, MCGPU_SEGMENT_STAGE_FINALIZE = 5 };
typedef struct mcgpu_segment_stage_args {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_stage_args); 0 is refused */
  int upsample;
  int c1, c2, c_out;
  int shape[3];
  int patch_shape[3];
  int n_patches;
  const int *starts;
  const float *in, *in2, *weight, *bias;
  void *out;
} mcgpu_segment_stage_args;
int mcgpu_segment_stage(const mcgpu_segment_options *options, int stage, const mcgpu_segment_stage_args *args, mcgpu_segment_report *report);

/* ------------------------------------------------------------------------------------------------
 * Training of the segmentation network on the device (what the reference obtains from cbctmc/segmentation/trainer.py:
 * CTSegmentationTrainer with the driver's SegmentationLoss(use_dice=True); csrc/segment_train.hip, whose header states the rule).
 * A trainer is a handle: the flat weights (the order of mcgpu_segment_options.weights), both Adam moments, both packings of the
 * weights and every buffer of a pass stay on the device between steps.  A batch is n <= max_batch samples: image, host float32
 * [n][P0][P1][P2], already rescaled, and target, host [n][9][P0][P1][P2], uint8 or float32 (target_type MCGPU_TARGET_*).
 *   p = softmax over channels 0..7 of the logits, sigmoid on channel 8 (float64, rounded once); per sample b and channel c
 *   I = sum t p, G = sum t, P = sum p (float64); f[b][c] = 1 - (2 I + 1e-5) / (G + P + 1e-5); loss = mean of f over b and c;
 *   loss_label[c] = mean of f over b.
 * Everything is float32 (the reference's trainer disables autocast for its forward pass; no gradient scaling).  The batch gradient
 * is the sum of the per-sample gradients in sample order; nothing is accumulated atomically: the same call gives the same bytes.
 * The bias of a convolution that feeds an instance norm has gradient exactly 0 by definition here and never
 * moves.  Adam as mcgpu_speedup_train_*; the learning rate is an argument of every step (the host's scheduler owns it).
 * Refused before any device call (-1, mcgpu_last_error): a null handle or array, n outside 1..max_batch, an unknown target_type,
 * lr <= 0 with update set; by mcgpu_segment_train_create: levels outside 1..8, filters outside 1..65535, n_classes other than 9,
 * filters or n_weights that do not fit together, a patch axis not divisible by 2^levels, a bottleneck of fewer than 2 voxels, a
 * patch of 2^31 voxels or more, betas out of range.
 * With `dry` set the handle is a plan: nothing touches the device, mcgpu_segment_train_get_state reports planned_device_bytes,
 * and calls that would run refuse after their other checks. */
typedef struct mcgpu_segment_trainer mcgpu_segment_trainer;
enum { MCGPU_TARGET_UINT8 = 0, MCGPU_TARGET_FLOAT32 = 1 };
typedef struct mcgpu_segment_train_options {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_train_options); 0 is refused */
  int device;
  int patch_shape[3];           /* samples are [P0][P1][P2], last axis fastest */
  int max_batch;                /* the largest n of a later call */
  int levels;                   /* 1..8; the reference's: 4 */
  int n_filters[18];            /* as mcgpu_segment_options; the reference's: 32 everywhere */
  int n_classes;                /* 9 */
  int dry;                      /* 1: plan only */
  const float *weights;         /* the initial flat weights */
  unsigned long long n_weights;
  double beta1, beta2;          /* 0.9, 0.999 */
} mcgpu_segment_train_options;
typedef struct mcgpu_segment_train_report {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_train_report) as the caller was compiled */
  int n;                        /* samples of the batch */
  double loss;                  /* mean of f over samples and labels */
  double loss_label[9];         /* mean of f over samples, by label (segmentation.LABELS) */
  unsigned long long step;      /* updates done so far: Adam's t */
  double ms_forward;            /* the copies of each sample to the device (they wait for it), the net, the Dice sums */
  double ms_wgrad;              /* weight- and bias-gradient kernels */
  double ms_dgrad;              /* head gradient, input-gradient kernels, their 2 x 2 x 2 sums, max-pool backward */
  double ms_norm;               /* backward of instance norm + LeakyReLU */
  double ms_optimizer;          /* Adam and the repacking of the weights */
  double ms_total;              /* wall time of the call */
  unsigned long long peak_device_bytes;  /* most device memory the trainer has held */
} mcgpu_segment_train_report;
typedef struct mcgpu_segment_train_state {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_train_state); 0 is refused */
  int reserved;
  float *weights, *moment1, *moment2;  /* host, [n_weights] each; a NULL array is not transferred */
  unsigned long long n_weights;
  unsigned long long step;      /* updates done: Adam's t */
  unsigned long long planned_device_bytes;  /* get: what the trainer holds (a dry handle: would hold) */
} mcgpu_segment_train_state;
int mcgpu_segment_train_create(const mcgpu_segment_train_options *options, mcgpu_segment_trainer **handle);
/* One batch.  update = 1: gradient of the loss, one Adam update with `lr`, both packings redone; update = 0: the losses alone
 * (the reference's validate_on_batch), nothing changes and lr is not read. */
int mcgpu_segment_train_step(mcgpu_segment_trainer *handle, int n, const float *image, const void *target, int target_type, double lr, int update,
                             mcgpu_segment_train_report *report);
/* The batch gradient of the loss, [n_weights] in the order of the flat weights; changes nothing. */
int mcgpu_segment_train_gradients(mcgpu_segment_trainer *handle, int n, const float *image, const void *target, int target_type, float *flat_gradient,
                                  mcgpu_segment_train_report *report);
/* logits [n][9][P0][P1][P2] of the trainer's forward pass with its present weights; changes nothing */
int mcgpu_segment_train_predict(mcgpu_segment_trainer *handle, int n, const float *image, float *logits);
/* Weights, moments and the step count, device -> host and back: a run resumed from them continues bit for bit.
 * set: n_weights must be the trainer's (unless all three arrays are NULL); the step count is always taken. */
int mcgpu_segment_train_get_state(mcgpu_segment_trainer *handle, mcgpu_segment_train_state *state);
int mcgpu_segment_train_set_state(mcgpu_segment_trainer *handle, const mcgpu_segment_train_state *state);
int mcgpu_segment_train_destroy(mcgpu_segment_trainer *handle);
/* One backward operator alone (for tests), on tensors [c][shape[0]][shape[1]][shape[2]]; all arrays are host float32 unless said.
 *   CONV_WGRAD: in [c1][shape], in2 [c2][shape2] or NULL (as MCGPU_SEGMENT_STAGE_CONV, `upsample` included), in3 = dY [c_out][shape]
 *     -> out = dW [c_out][c1 + c2][3][3][3], out2 = db [c_out] (may be NULL); values[0] = number of partials.
 *   CONV_DGRAD: in = dY [c_out][shape], in2 = weight [c_out][c1 + c2][3][3][3] -> out = d in [c1][shape], out2 = d in2 [c2][shape2]
 *     (c2 > 0; with `upsample` the sum over each 2 x 2 x 2 block).
 *   MAXPOOL_BACKWARD: in = x [c1][shape], in2 = dy [c1][shape / 2], in3 = what dx holds before, [c1][shape], or NULL for zeros
 *     -> out = dx.
 *   LOSS: in = logits [n][9][shape], in2 = target [n][9][shape] -> out = dL/d logits [n][9][shape] of the batch loss, values =
 *     double [1 + 9 n]: the loss, then f [n][9]. */
enum { MCGPU_SEGMENT_TRAIN_STAGE_CONV_WGRAD = 0, MCGPU_SEGMENT_TRAIN_STAGE_CONV_DGRAD = 1, MCGPU_SEGMENT_TRAIN_STAGE_MAXPOOL_BACKWARD = 2,
       MCGPU_SEGMENT_TRAIN_STAGE_LOSS = 3 };
typedef struct mcgpu_segment_train_stage_args {
  unsigned int struct_size;     /* sizeof(mcgpu_segment_train_stage_args); 0 is refused */
  int device;
  int shape[3];
  int upsample, c1, c2, c_out;
  const float *in, *in2, *in3;
  float *out, *out2;
  double *values;
  unsigned long long n;         /* LOSS: samples */
} mcgpu_segment_train_stage_args;
int mcgpu_segment_train_stage(int stage, const mcgpu_segment_train_stage_args *args, mcgpu_segment_train_report *report);

#ifdef __cplusplus
}
#endif
#endif /* MCGPU_AMD_H_ */
