// tally_stage.hpp -- staging of the detector tally of the FAST kernel: the mapping of tally words to bins, shared by the host (plan,
// C ABI query) and the device (producer in track_pool.inc, fold in tally_fold.hip).
//
// The tally is 4 planes (scatter classes) of `pixels` 64-bit words.  A detected photon used to cost one scattered 64-bit atomic at
// the memory side; staged, it costs one LDS add and one plain 8-byte store of a RECORD into a block of memory that belongs to
// (workgroup, bin), and a second kernel sums each bin's records in LDS and touches every tally word once.
//   * pixels are dealt to the bins in RUNS of 64 consecutive pixels (512 bytes of a plane), round-robin:
//       run = pixel / 64,  bin = run % n_bins,  offset = (run / n_bins) * 64 + pixel % 64
//     so every bin samples the whole detector (open field and the object's shadow alike) and one capacity fits all bins;
//   * a bin holds its pixels in all four planes: bin-relative word = plane * bin_pixels + offset  (< words_per_bin = 4 * bin_pixels);
//   * a record is {value = round(E * 100) in the low dword, bin-relative word in the high dword}.
// Integer sums commute: the image is the same, bit for bit, as with the direct atomics.
//
// The second tally `w2` (same shape as the image, uint64; null = off): a history that scores w in word i also adds (w >> 10)^2 to
// w2[i] -- tally_w2_term below, one definition for the COMPAT kernel, the FAST kernels' direct add and the fold's squares pass (which
// reads the same records), and the CPU oracle's.  w <= 1.25e7 (125 keV in 0.01 eV), so a term is at most 12207^2 = 1.5e8 and 2^64 holds
// 1.2e11 of the largest terms in ONE word: no history count the engine accepts can overflow a sum.  The shift drops at most
// 2 * 1024 / w of a term: 0.4 % at w_min = 5e5 (the 5 keV floor of the tables), 0.03 % at the mean energy.  A history scores at most
// one word, so sums of w2 over any set of words (a scatter class, a block, the detector) are the second moments of that set's score.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MC_STAGE_HD __host__ __device__
#else
#define MC_STAGE_HD
#endif

namespace mcgpu {

constexpr unsigned int kTallyW2Shift = 10;       // w2 += (w >> kTallyW2Shift)^2
constexpr unsigned int kStageRun = 64;           // pixels of a run
constexpr unsigned int kStageRunsPerBin = 64;    // a bin's words as 64-bit counters fill at most 128 KiB of the fold's LDS
constexpr int kStageExteriorPercent = 50;        // default rule: stage where at least this share of the bricks is exterior (engine_launch.cpp: TallyStage::wanted)
constexpr unsigned int kStageCapSlack = 16;      // records added to every block's capacity
// Histories a workgroup may run beyond its even share of the launch: history ids are dealt in chunks of 256 per wave (track_common.inc:
// kChunk), and in a launch of few chunks the waves that ask first get them all -- a workgroup of 16 waves then holds one or two chunks
// per wave whatever the mean share is.  Two chunks per wave; negligible beside the share of a large launch (1e8 histories: 3 %).
constexpr unsigned int kStageWorkgroupSlack = 2u * 16u * 256u;

MC_STAGE_HD inline unsigned long long tally_w2_term(unsigned long long w) { return (w >> kTallyW2Shift) * (w >> kTallyW2Shift); }

struct TallyStagePlan {
  unsigned int pixels;         // pixels of one plane
  unsigned int n_bins;         // 0: no staging for this detector
  unsigned int bin_pixels;     // pixels of a bin (runs of the fullest bin * 64)
  unsigned int words_per_bin;  // 4 * bin_pixels
  unsigned int magic;          // ceil(2^32 / n_bins): run / n_bins = umulhi(run, magic), exact while runs * n_bins < 2^32
  unsigned int cap;            // records per (workgroup, bin)
  unsigned int workgroups;
  unsigned long long bytes;    // cap * workgroups * n_bins * 8
};

// `bins` = 0: as few bins as kStageRunsPerBin allows; `cap` = 0: from the histories of the launch.
inline TallyStagePlan tally_stage_plan(unsigned long long detector_words, unsigned long long histories, unsigned int workgroups, unsigned int bins,
                                       unsigned int cap) {
  TallyStagePlan P{};
  const unsigned long long pixels = detector_words / 4ULL;
  if (pixels == 0 || pixels >= (1ULL << 30) || workgroups == 0) return P;
  const unsigned long long runs = (pixels + kStageRun - 1) / kStageRun;
  const unsigned long long n_bins = bins ? bins : (runs + kStageRunsPerBin - 1) / kStageRunsPerBin;
  if (n_bins >= (1ULL << 16) || runs * n_bins >= (1ULL << 32)) return P;
  const unsigned long long runs_per_bin = (runs + n_bins - 1) / n_bins;
  P.pixels = (unsigned int)pixels;
  P.n_bins = (unsigned int)n_bins;
  P.bin_pixels = (unsigned int)(runs_per_bin * kStageRun);
  P.words_per_bin = 4u * P.bin_pixels;
  P.magic = (unsigned int)(((1ULL << 32) + n_bins - 1) / n_bins);  // n_bins = 1: 2^32 wraps to 0, handled by stage_split
  P.workgroups = workgroups;
  const unsigned long long streams = (unsigned long long)workgroups * n_bins;
  // per workgroup 1.25 x its even share (a history scores at most once; the bins see the same mix of pixels, and 25 % is six sigma of
  // the 560 hits a block expects at 1e8 histories and a detection rate of one) + kStageWorkgroupSlack, spread over the bins
  const unsigned long long per_workgroup = (5ULL * histories + 4ULL * workgroups - 1) / (4ULL * workgroups) + kStageWorkgroupSlack;
  unsigned long long c = cap ? cap : (per_workgroup + n_bins - 1) / n_bins + kStageCapSlack;
  c = (c + 1ULL) & ~1ULL;  // blocks of whole 16 bytes
  if (c >= (1ULL << 31)) { P.n_bins = 0; return P; }
  P.cap = (unsigned int)c;
  P.bytes = c * streams * 8ULL;
  return P;
}

// run -> (bin, run of the bin)
MC_STAGE_HD inline void stage_split(unsigned int run, unsigned int n_bins, unsigned int magic, unsigned int& bin, unsigned int& bin_run) {
#if defined(__HIP_DEVICE_COMPILE__)
  bin_run = (n_bins == 1u) ? run : __umulhi(run, magic);
#else
  bin_run = (n_bins == 1u) ? run : (unsigned int)(((unsigned long long)run * magic) >> 32);
#endif
  bin = run - bin_run * n_bins;
}

// tally word (plane * pixels + pixel) -> bin and bin-relative word
MC_STAGE_HD inline void stage_map(unsigned int word, unsigned int pixels, unsigned int n_bins, unsigned int magic, unsigned int bin_pixels, unsigned int& bin,
                                  unsigned int& rel) {
  const unsigned int plane = (word >= pixels ? 1u : 0u) + (word >= 2u * pixels ? 1u : 0u) + (word >= 3u * pixels ? 1u : 0u);
  const unsigned int pixel = word - plane * pixels;
  unsigned int bin_run;
  stage_split(pixel / kStageRun, n_bins, magic, bin, bin_run);
  rel = plane * bin_pixels + bin_run * kStageRun + (pixel % kStageRun);
}

// bin-relative word -> tally word, or 0xFFFFFFFF for the padding of a bin (no pixel there)
MC_STAGE_HD inline unsigned int stage_unmap(unsigned int bin, unsigned int rel, unsigned int pixels, unsigned int n_bins, unsigned int bin_pixels) {
  const unsigned int plane = (rel >= bin_pixels ? 1u : 0u) + (rel >= 2u * bin_pixels ? 1u : 0u) + (rel >= 3u * bin_pixels ? 1u : 0u);
  const unsigned int off = rel - plane * bin_pixels;
  const unsigned long long pixel = ((unsigned long long)(off / kStageRun) * n_bins + bin) * kStageRun + (off % kStageRun);
  return pixel < pixels ? plane * pixels + (unsigned int)pixel : 0xFFFFFFFFu;
}

// Sub-launches of a launch of `count` histories from `first`: range k of ceil(count / limit) (count = 0: one empty range)
inline void stage_sub_launch(unsigned long long first, unsigned long long count, unsigned long long limit, unsigned long long k, unsigned long long& sub_first,
                             unsigned long long& sub_count) {
  const unsigned long long at = k * limit;
  sub_first = first + (at < count ? at : count);
  sub_count = at < count ? (count - at < limit ? count - at : limit) : 0ULL;
}
inline unsigned long long stage_sub_launches(unsigned long long count, unsigned long long limit) { return count == 0 ? 1ULL : (count + limit - 1) / limit; }

// What the FAST kernels and the fold read (TrackArgs::stage): region == null selects the direct atomics
struct StageArgs {
  unsigned long long* region;    // records: [(workgroup * n_bins + bin) * cap + slot]
  unsigned int* counts;          // records written per (workgroup, bin): [workgroup * n_bins + bin]; every launched workgroup writes all of its entries, nothing clears them
  unsigned long long* fallback;  // hits that took the direct atomic (all launches since the last reset)
  unsigned int pixels, n_bins, magic, bin_pixels, cap;
  int cursor;                    // byte offset of the workgroup's cursors in the LDS image: u32[n_bins], then the fallback counter
};

}  // namespace mcgpu
