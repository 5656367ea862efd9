// tally_fold.hip -- second half of the staged detector tally (tally_stage.hpp): sums the records the FAST kernel stored per
// (workgroup, bin) and adds each bin's sums to the image.
//
// One workgroup per bin.  The bin's words live in LDS as 64-bit counters (4 planes x bin_pixels, at most 128 KiB); the blocks of the
// producing workgroups are spread over the waves, read with 16-byte loads (a block starts on 16 bytes: the capacity is even) and
// added with ds_add_u64.  Then every non-zero counter is added to its tally word with a plain load, add and store: bins are
// disjoint, the fold runs in the stream behind the track kernel, and that kernel's own (fallback) atomics are complete at the
// kernel boundary.  A launch that tallies squared weights runs the same walk a second time over the same records with kSquares, adding
// tally_w2_term(value) into the same counters and those into `w2`: a second launch, not a second counter set in one kernel -- two sets
// are 256 KiB at the plan's largest bin (4096 pixels; 160 KiB of LDS hold both only up to 2560), and the plain fold stays the
// instruction stream it was (profiles/tally_variance_ab.md).  The name keeps clear of "track_..._kernel", the pattern by which the PMC tools select the track kernel's rows.
#include <hip/hip_runtime.h>

#include "tally_stage.hpp"

namespace mcgpu {
namespace {

constexpr int kFoldThreads = 1024;
extern __shared__ __attribute__((aligned(16))) unsigned long long fold_lds[];

template <bool kSquares>
__device__ __forceinline__ void fold_add(unsigned long long record, unsigned int words) {
  const unsigned int rel = (unsigned int)(record >> 32);
  const unsigned long long value = record & 0xFFFFFFFFULL;
  if (rel < words) atomicAdd(fold_lds + rel, kSquares ? tally_w2_term(value) : value);
}

template <bool kSquares>
__global__ __launch_bounds__(kFoldThreads) void tally_stage_fold(const StageArgs S, const unsigned int workgroups, unsigned long long* __restrict__ image) {
  const unsigned int bin = blockIdx.x, words = 4u * S.bin_pixels;
  for (unsigned int i = threadIdx.x; i < words; i += kFoldThreads) fold_lds[i] = 0ULL;
  __syncthreads();
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  constexpr unsigned int kWaves = kFoldThreads / 64;
  // 64 blocks per wave and pass: lane l first fetches the count of block g0 + l * kWaves, so that the record loads of the pass do not
  // each wait for a count of their own.  The blocks are then taken four at a time with all their loads issued before the first add
  // (a block of the headline launch holds 420 records = 3.3 pairs per lane): one memory round trip per four blocks, not per block.
  constexpr unsigned int kGroup = 4, kDeep = 4;
  for (unsigned int g0 = wave; g0 < workgroups; g0 += 64u * kWaves) {
    const unsigned int g_mine = g0 + lane * kWaves;
    const unsigned int n_mine = g_mine < workgroups ? min(S.counts[(size_t)g_mine * S.n_bins + bin], S.cap) : 0u;
    for (unsigned int l0 = 0; l0 < 64u && g0 + l0 * kWaves < workgroups; l0 += kGroup) {
      ulonglong2 r[kGroup][kDeep];
      unsigned int n[kGroup];
      const unsigned long long* src[kGroup];
#pragma unroll
      for (unsigned int u = 0; u < kGroup; ++u) {
        n[u] = (unsigned int)__builtin_amdgcn_readlane((int)n_mine, (int)(l0 + u));  // 0 beyond the last block
        const unsigned int g = min(g0 + (l0 + u) * kWaves, workgroups - 1u);
        src[u] = S.region + (size_t)(g * S.n_bins + bin) * S.cap;
        const ulonglong2* const src2 = reinterpret_cast<const ulonglong2*>(src[u]);
#pragma unroll
        for (unsigned int j = 0; j < kDeep; ++j) {
          const unsigned int i = lane + 64u * j;
          r[u][j] = make_ulonglong2(~0ULL, ~0ULL);  // a record no bin holds: fold_add ignores it
          if (i < (n[u] >> 1)) r[u][j] = src2[i];
        }
      }
#pragma unroll
      for (unsigned int u = 0; u < kGroup; ++u) {
#pragma unroll
        for (unsigned int j = 0; j < kDeep; ++j) {
          fold_add<kSquares>(r[u][j].x, words);
          fold_add<kSquares>(r[u][j].y, words);
        }
        const ulonglong2* const src2 = reinterpret_cast<const ulonglong2*>(src[u]);
        for (unsigned int i = lane + 64u * kDeep; i < (n[u] >> 1); i += 64u) {  // blocks beyond 512 records
          const ulonglong2 a = src2[i];
          fold_add<kSquares>(a.x, words);
          fold_add<kSquares>(a.y, words);
        }
        if ((n[u] & 1u) != 0u && lane == 0u) fold_add<kSquares>(src[u][n[u] - 1u], words);
      }
    }
  }
  __syncthreads();
  for (unsigned int i = threadIdx.x; i < words; i += kFoldThreads) {
    const unsigned long long v = fold_lds[i];
    if (v == 0ULL) continue;
    const unsigned int w = stage_unmap(bin, i, S.pixels, S.n_bins, S.bin_pixels);
    if (w != 0xFFFFFFFFu) image[w] += v;
  }
}

}  // namespace

// LDS of a fold workgroup; more than 64 KiB needs the attribute once per process and device
hipError_t prepare_tally_fold(const StageArgs& S) {
  const size_t lds = (size_t)4 * S.bin_pixels * 8;
  if (lds <= 64 * 1024) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tally_stage_fold<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&tally_stage_fold<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t launch_tally_fold(const StageArgs& S, unsigned int workgroups, unsigned long long* image, hipStream_t stream) {
  hipLaunchKernelGGL(tally_stage_fold<false>, dim3(S.n_bins), dim3(kFoldThreads), (size_t)4 * S.bin_pixels * 8, stream, S, workgroups, image);
  return hipGetLastError();
}

// the squares of the same records into `w2`
hipError_t launch_tally_fold_squares(const StageArgs& S, unsigned int workgroups, unsigned long long* w2, hipStream_t stream) {
  hipLaunchKernelGGL(tally_stage_fold<true>, dim3(S.n_bins), dim3(kFoldThreads), (size_t)4 * S.bin_pixels * 8, stream, S, workgroups, w2);
  return hipGetLastError();
}

}  // namespace mcgpu
