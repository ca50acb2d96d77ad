// log_ring.h -- where the log ring of a kv engine (tatp / smallbank) stands: the two tail words, the count of records ever
// appended and the drain cursor, and what a pass's partition stage, a cancelled announcement and a drain do to them.  One
// source for the engine (engine.hip: ahead_cancel, log_drain_locked), the partition stage (k_kv_dev.h, kv_part_body) and the
// host form (dint_log_ring_host, include/dint_driver.h), as log_replay.h is for the replay.
//
//   tail[2]    ring positions.  The partition of pass p reads tail[p & 1] and writes tail[(p + 1) & 1]: it may run beside the
//              resolve stage of pass p - 1 (dint_submit_device_ahead), so the position "before" and "after" are two words.
//   appended   records ever appended (64 bits): record k of the stream lives at ring slot k % cap.
//   drained    the drain cursor (host side): records handed out, or given up as lost, so far.
//   gone       (host side) records that a cancelled batch overwrote while they were still to be drained.
//
// A cancelled announcement (include/dint_abi.h, dint_submit_device_ahead) leaves all four as if the announced batch had never
// been seen.  What it takes back is the batch's own count of log records, which the partition stage left in a control word --
// NOT the distance of the two tail words: a batch of exactly `cap` records moves the tail once round the ring, a distance of 0.
// The cursor comes back with the count: records drained between announcement and cancel were the caller's to discard, and the
// record appended next is the next one drained.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LG_HD __host__ __device__
#else
#define LG_HD
#endif

struct LgRing {
  uint32_t tail[2];
  uint64_t appended, drained;
  uint64_t gone;  // records a cancelled batch overwrote before they were drained: the next drain reports them as lost
};

// the ring position `total` records behind `tail`
LG_HD static inline uint32_t lg_tail_after(uint32_t tail, uint32_t total, uint32_t cap) {
  return (uint32_t)(((uint64_t)tail + total) % cap);
}

// the tail word that says where the ring stands after pass number `pass_no` (the last one launched): the one that pass wrote.
// An announced pass pass_no + 1 reads it and writes the other one, so dint_read_log's tail does not include an announced batch.
static inline uint32_t lg_cur(uint64_t pass_no) { return (uint32_t)((pass_no + 1) & 1); }

// the partition stage of a pass with `total` log records; rd = the tail word it reads (pass number & 1)
static inline void lg_append(LgRing &r, uint32_t rd, uint32_t total, uint32_t cap) {
  r.tail[rd ^ 1u] = lg_tail_after(r.tail[rd], total, cap);
  r.appended += total;
}

// the announced pass whose partition appended `total` records will not be answered; rd = the tail word it read
static inline void lg_cancel(LgRing &r, uint32_t rd, uint32_t total, uint32_t cap) {
  if (r.appended - r.drained > cap) {  // the batch lapped the reader: what it overwrote is gone although it is taken back itself
    const uint64_t over = r.appended - r.drained - cap;
    r.drained += over;
    r.gone += over;
  }
  r.tail[rd ^ 1u] = r.tail[rd];
  r.appended -= total < r.appended ? total : r.appended;
  if (r.drained > r.appended) r.drained = r.appended;
}

// a drain into room for `room` records: n records from ring slot pos on (wrapping at cap), `lost` given up before them
struct LgDrain {
  uint64_t pos, n, lost;
};
static inline LgDrain lg_drain(LgRing &r, uint32_t cap, uint64_t room) {
  LgDrain d = {0, 0, 0};
  if (r.drained > r.appended) r.drained = r.appended;  // the engine was reset / restored to an earlier state
  uint64_t pending = r.appended - r.drained;
  if (pending > cap) {  // the ring lapped the reader: the oldest records are overwritten
    d.lost = pending - cap;
    pending = cap;
  }
  r.drained += d.lost;
  d.lost += r.gone;
  r.gone = 0;
  d.n = pending < room ? pending : room;
  d.pos = r.drained % cap;
  r.drained += d.n;
  return d;
}

// ---- the host form (dint_log_ring_host, include/dint_driver.h): a walk over the calls above ------------------------------------------------
// ops = n_ops pairs {code, arg}; the ring holds record ids (1, 2, 3 .. in the order the partition stages appended them, cancelled
// ones included).  After every op four words go to `out`: {dint_read_log's tail, appended, drained, the other tail word}; a DRAIN
// adds {n, lost, the n ids}.  Returns the words written, or -1: a bad op, a sequence no engine allows, `out` too small.
enum { LG_OP_PASS = 0, LG_OP_ANNOUNCE = 1, LG_OP_KEEP = 2, LG_OP_CANCEL = 3, LG_OP_DRAIN = 4 };
static inline int64_t lg_walk(uint32_t cap, const uint32_t *ops, uint32_t n_ops, uint64_t *out, uint64_t out_cap) {
  if (!cap || (n_ops && (!ops || !out))) return -1;
  LgRing r = {{0, 0}, 0, 0, 0};
  uint64_t *ring = new uint64_t[cap]();
  uint64_t pass_no = 0, next_id = 1, w = 0;
  uint32_t pending = 0;
  bool announced = false, ok = true;
  auto append = [&](uint64_t p, uint32_t total) {  // the partition of pass p: records behind tail[p & 1], then the words
    for (uint32_t i = 0; i < total; i++) ring[lg_tail_after(r.tail[p & 1], i, cap)] = next_id++;
    lg_append(r, (uint32_t)(p & 1), total, cap);
  };
  for (uint32_t k = 0; k < n_ops && ok; k++) {
    const uint32_t op = ops[2 * k], arg = ops[2 * k + 1];
    uint64_t extra[2] = {0, 0};
    LgDrain d = {0, 0, 0};
    switch (op) {
      case LG_OP_PASS:  // a plain pass of `arg` log records (a pass is clamped to the ring: arg <= cap)
        ok = !announced && arg <= cap;
        if (ok) append(++pass_no, arg);
        break;
      case LG_OP_ANNOUNCE:  // the partition of the next pass rides in this one's launch
        ok = !announced && arg <= cap && pass_no > 0;
        if (ok) { append(pass_no + 1, arg); announced = true; pending = arg; }
        break;
      case LG_OP_KEEP:  // the announced pass is submitted: it is the last one launched now
        ok = announced;
        if (ok) { pass_no++; announced = false; }
        break;
      case LG_OP_CANCEL:
        ok = announced;
        if (ok) { lg_cancel(r, lg_cur(pass_no), pending, cap); announced = false; }
        break;
      case LG_OP_DRAIN:
        d = lg_drain(r, cap, arg);
        extra[0] = d.n; extra[1] = d.lost;
        break;
      default:
        ok = false;
    }
    if (!ok || w + 4 + (op == LG_OP_DRAIN ? 2 + d.n : 0) > out_cap) { ok = false; break; }
    out[w++] = r.tail[lg_cur(pass_no)]; out[w++] = r.appended; out[w++] = r.drained; out[w++] = r.tail[lg_cur(pass_no) ^ 1u];
    if (op == LG_OP_DRAIN) {
      out[w++] = extra[0]; out[w++] = extra[1];
      for (uint64_t i = 0; i < d.n; i++) out[w++] = ring[(d.pos + i) % cap];
    }
  }
  delete[] ring;
  return ok ? (int64_t)w : -1;
}
