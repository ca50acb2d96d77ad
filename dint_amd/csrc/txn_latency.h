// txn_latency.h -- latency of the closed-loop clients' transactions, one rule for the host driver (txn_driver.cc) and
// the GPU-resident driver (k_txn.hip); include/dint_driver.h struct dint_driver_latency.
//
// The reference's TATP / SmallBank clients keep one latency sample per COMMITTED transaction and print average, median,
// 99th and 99.9th percentile at the end of a run (tatp/caladan/client_udp_shard.cc:94-107, :1148-1182, Percentile() of
// tatp/caladan/stat.h:12-17).  The drivers here are epoch-synchronous, so a transaction's latency has two measures:
//
//   ROUND TRIPS  r = the number of epochs in which the transaction emitted messages (one epoch = one send-and-await-all-
//                replies phase).  A transaction that begins inside the emit of epoch b and is finished inside the emit
//                of epoch f has r = f - b.  The client header counts it in a byte that was padding (tx_rt_count
//                below): when tatp_run / sb_run returns with the phase's messages the byte is incremented, from zero if
//                the phase began a transaction (tatp_begin / sb_begin ran), and TxOut::finish reports it -> fin_rt[].
//                (The zero is not stored inside tatp_begin itself: there the store changed the register allocation of
//                the whole device kernel; taken as a flag to where the byte is written anyway, it does not.)  A phase
//                whose messages found no room in a full batch still counts: the client waited an epoch for them.
//   TICKS        (GPU driver only) the device's constant-rate clock.  The emit kernel of epoch e leaves one stamp in slot
//                e & (LAT_RING - 1) of a ring; a transaction of r round trips that finished in epoch e has latency
//                now - ring[(e - r) & (LAT_RING - 1)], `now` read once per workgroup.  Kept as a log-linear histogram
//                (lat_tick_bin): values below 16 map to themselves, above that 8 sub-bins per power of two (a bin is at
//                most 12.5 % wide), the last bin saturates.  LAT_TICK_BINS covers 2^32 ticks: 42 s at the 100 MHz the
//                CDNA parts report, one second at any rate up to 4 GHz.
//
// Aborted transactions are counted too, in arrays of their own (round trips only): an extension, the reference drops them.
#pragma once
#include <stdint.h>

#include "../../include/dint_driver.h"

#if defined(__HIPCC__)
#define LAT_HD __host__ __device__
#else
#define LAT_HD
#endif

#define LAT_RT_BINS DINT_LAT_RT_BINS      // round trips are binned as min(r, LAT_RT_BINS - 1)
#define LAT_TICK_BINS DINT_LAT_TICK_BINS
#define LAT_RING 256u                     // epoch stamps kept: one more than the largest r the header's byte can hold
static_assert(LAT_TICK_BINS == 16 + 8 * 28, "16 linear bins, then 8 per power of two from 2^4 to 2^31");
static_assert((LAT_RING & (LAT_RING - 1)) == 0 && LAT_RING > 255, "a power of two above the saturated round-trip count");

// the round-trip byte of a client header after a phase that emitted messages: one more, from zero if the phase began the
// transaction; saturates at 255
LAT_HD static inline void tx_rt_count(uint8_t &rt, bool began) {
  const uint8_t r = began ? (uint8_t)0 : rt;
  rt = (uint8_t)(r + (r != 255));
}

LAT_HD static inline uint32_t lat_rt_bin(uint32_t r) { return r < LAT_RT_BINS - 1 ? r : LAT_RT_BINS - 1; }

LAT_HD static inline uint32_t lat_tick_bin(uint64_t ticks) {
  if (ticks < 16) return (uint32_t)ticks;
  const uint32_t e = 63u - (uint32_t)__builtin_clzll(ticks);  // floor(log2(ticks)) >= 4
  const uint32_t bin = 16 + (e - 4) * 8 + (uint32_t)((ticks >> (e - 3)) & 7);
  return bin < LAT_TICK_BINS - 1 ? bin : LAT_TICK_BINS - 1;
}
// the smallest value of a bin (bin = LAT_TICK_BINS: where the last bin would end if it did not saturate)
LAT_HD static inline uint64_t lat_tick_bin_lo(uint32_t bin) {
  if (bin < 16) return bin;
  const uint32_t e = 4 + (bin - 16) / 8, sub = (bin - 16) % 8;
  return e - 3 < 61 ? (uint64_t)(8 + sub) << (e - 3) : ~0ull;
}

// one finished transaction into the round-trip fields (the host driver; the GPU driver goes through LDS counters)
static inline void lat_add_round_trips(dint_driver_latency *L, uint8_t txn, bool committed, uint8_t r) {
  txn &= 7;
  if (!committed) { L->aborted_round_trips[txn][lat_rt_bin(r)]++; return; }
  L->round_trips[txn][lat_rt_bin(r)]++;
  L->rt_sum[txn] += r;
  if (r > L->rt_max[txn]) L->rt_max[txn] = r;
}
