// id_tickets.hpp -- how the FAST kernel's history ids are dealt: the split of a launch over the id dispensers, the ticket schedule of a
// dispenser and the walk over the dispensers at the end of a launch.  Pure integer functions shared by the device (track_pool.inc:
// deal_history_ids) and the host (C ABI queries mcgpu_id_tickets / mcgpu_id_next_counter, tests/test_id_tickets.py).
//
// A launch of `count` ids (0 .. count-1, relative to its first history) is cut into kNumCounters contiguous parts, one per dispenser.
// A dispenser is a TICKET counter (the low dword of its 64-bit word, atomicAdd 1: the engine refuses launches whose ticket numbers
// could pass 2^32): ticket t of a dispenser of `size` ids is the fixed range t * kIdChunk .. (t + 1) * kIdChunk - 1 of that part,
// cut at the part's end and empty from there on: a wave that draws an empty ticket has found the dispenser exhausted.  (Finer
// tickets towards the end of a part -- 16, 32 or 64 ids over the last 4096 to 16384 -- were measured and do not shorten the launch:
// profiles/launch_end_ab.md.  The mapping is the place to try another schedule; no ticket may exceed kIdChunk.)
//
// One more word of the dispenser block, the EXHAUSTION MASK, holds one bit per dispenser: set (by a non-returning atomic OR on the
// bit's dword) by a wave that drew an empty ticket from it, never cleared during a launch, zeroed with the block before the next.  A
// wave reads it only after an empty ticket of its own and then asks only dispensers whose bit is clear; a bit it does not see yet
// merely costs it one more empty ticket.  Nothing waits on the mask.
#pragma once

#if defined(__HIPCC__)
#define MC_ID_HD __host__ __device__
#else
#define MC_ID_HD
#endif

namespace mcgpu {

constexpr int kNumCounters = 64, kCounterStride = 32;  // FAST: history-id dispensers (u64 each, 256 B apart)
constexpr unsigned int kIdChunk = 256;                 // ids of a ticket (tally_stage.hpp: kStageWorkgroupSlack allows two per wave)
// the exhaustion mask: a word of the padding between dispenser 0 and dispenser 1, in the 128-byte line that holds no dispenser
constexpr int kIdMaskWord = 16;
static_assert(kIdMaskWord > 0 && kIdMaskWord < kCounterStride && kNumCounters <= 64, "the mask sits in the padding and holds a bit per dispenser");

// the part of a launch of `count` ids that dispenser `ctr` owns: ids base .. base + size - 1
MC_ID_HD inline void id_counter_part(unsigned long long count, unsigned int ctr, unsigned long long& base, unsigned long long& size) {
  const unsigned long long q = count / kNumCounters, r = count % kNumCounters;
  base = q * ctr + (ctr < r ? (unsigned long long)ctr : r);
  size = q + (ctr < r ? 1ULL : 0ULL);
}

// all non-empty tickets of a dispenser of `size` ids
MC_ID_HD inline unsigned long long id_ticket_count(unsigned long long size) { return size / kIdChunk + (size % kIdChunk ? 1ULL : 0ULL); }

// ticket t of a dispenser of `size` ids: ids lo .. hi - 1 of its part (lo == hi: empty, the dispenser is exhausted)
MC_ID_HD inline void id_ticket_range(unsigned long long size, unsigned long long t, unsigned long long& lo, unsigned long long& hi) {
  if (t >= id_ticket_count(size)) {  // compared as a ticket number: t * kIdChunk may not fit
    lo = hi = size;
    return;
  }
  lo = t * kIdChunk;
  hi = lo + kIdChunk < size ? lo + kIdChunk : size;
}

// The dispenser to ask after `ctr`: the first one after it, cyclically, whose bit in `mask` is clear (ctr itself comes last), or
// kNumCounters when every bit is set.
MC_ID_HD inline unsigned int id_next_counter(unsigned long long mask, unsigned int ctr) {
  const unsigned int s = (ctr + 1u) % (unsigned int)kNumCounters;
  const unsigned long long clear = ~((mask >> s) | (s ? mask << (kNumCounters - s) : 0ULL));  // bit k: dispenser (s + k) % 64 is not known to be exhausted
  if (clear == 0ULL) return (unsigned int)kNumCounters;
  unsigned int k = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  k = (unsigned int)__ffsll((long long)clear) - 1u;
#else
  while (!((clear >> k) & 1ULL)) ++k;
#endif
  return (s + k) % (unsigned int)kNumCounters;
}

}  // namespace mcgpu
