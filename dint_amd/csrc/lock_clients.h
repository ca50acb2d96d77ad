// lock_clients.h -- the lock micro-benchmarks' load generators, one source for the host clients (fasst_client.cc,
// tpl_client.cc) and the GPU-resident client (k_lock_client.hip), as txn_clients.h is for tatp / smallbank.
//
// lock_fasst  lock_fasst/caladan/client.cc:183-280 (ClientLoop) over transactions shaped like trace_init.sh:6-27
// lock_2pl    lock_2pl/caladan/client.cc:167-240 (ClientLoop) over transactions shaped like trace_init.sh:6-27
// Both draw a transaction the same way: 5..10 distinct keys (random.sample), sorted, and per key in sorted order one
// draw `rnd % 100 >= read_pct` that makes it a write key (FaSST) / an exclusive lock (2PL), from the reference's own LCG
// (`fastrand`, tatp/caladan/tatp.h:31-34) seeded 0xdeadbeef + worker; keys uniform over the key space or Zipf(theta)
// (zipf_table.h).  A worker has ONE request outstanding; W workers run in lock step (one EPOCH = every worker's next
// request, in worker order).
//
// A worker's state is a one-dword header (LcState packed) + its RNG + the transaction's keys (+ the versions it read,
// FaSST).  The state machines reach keys / versions / RNG only through a storage object S, so the host keeps a worker
// in a struct (LcWorker) and the device keeps it in dword columns of HBM: per request a lane touches its header and the
// key or version the step needs; the key set and the RNG are touched only when a transaction starts.
// Everything here is integer arithmetic with no library calls, so host and device produce the same bytes.
#pragma once
#include <stdint.h>

#include "zipf_table.h"

#if defined(__HIPCC__)
#define LC_HD __host__ __device__
#else
#define LC_HD
#endif

#pragma pack(push, 1)
struct FasstMsg {  // lock_fasst/caladan/proto.h:31-36 (= lock_fasst/udp/net.h:23-29)
  uint8_t type;
  uint32_t lid;
  uint32_t ver;
};
struct TplMsg {  // lock_2pl/caladan/proto.h:27-31 (= lock_2pl/udp/net.h:25-31)
  uint8_t action;
  uint32_t lid;
  uint8_t type;
};
#pragma pack(pop)
static_assert(sizeof(FasstMsg) == 9 && sizeof(TplMsg) == 6, "packed wire structs");

enum : uint8_t { F_READ = 0, F_ACQ = 1, F_ABORT = 2, F_COMMIT = 3, F_GRANT_READ = 4, F_GRANT_LOCK = 5, F_REJECT_LOCK = 6 };
enum : uint8_t { L_ACQUIRE = 0, L_RELEASE = 1, L_GRANT = 2, L_REJECT = 3, L_RELEASE_ACK = 5 };  // lock_2pl PktType
// FaSST phases
enum : uint32_t { P_READ, P_ACQ, P_REJ_ABORT, P_VALIDATE, P_RB_ABORT, P_COMMIT };
// 2PL modes: acquire in ascending order / release what is held after a REJECT (acquisition order) / release all (reverse)
enum : uint32_t { M_ACQ, M_ROLL, M_REL };

#define LC_MAXK 10u  // keys of a transaction at most

// what a consume step reports (bits): the worker's transaction committed, a REJECT, a validation failure (FaSST), a reply
// the reference client would assert / panic on (lid / type: up to two protocol errors)
#define LC_EV_COMMIT 1u
#define LC_EV_REJECT 2u
#define LC_EV_ROLLBACK 4u
#define LC_EV_PERR_LID 8u
#define LC_EV_PERR_TYPE 16u

struct LcParams {
  uint32_t key_space;        // keys are drawn from [0, key_space)
  uint32_t read_pct;         // a key is a read key / shared lock with this probability (percent)
  uint32_t key_dist;         // 0 = uniform, 1 = Zipf (zipf_cdf)
  uint32_t reserved;
  uint64_t zipf_n;           // = key_space
  const uint32_t *zipf_cdf;  // ZipfTable::cdf (host or device memory, matching the caller)
};

// the header: phase / mode (3 bits), pos (4), nk (4), aux (4: FaSST the locks to ABORT after a REJECT, 2PL the locks
// held), wmask (10: key j of the sorted set is a write key / exclusive)
struct LcState {
  uint32_t phase, pos, nk, aux, wmask;
};
LC_HD inline LcState lc_unpack(uint32_t h) {
  return {h & 7u, (h >> 3) & 15u, (h >> 7) & 15u, (h >> 11) & 15u, (h >> 15) & 1023u};
}
LC_HD inline uint32_t lc_pack(const LcState &s) {
  return s.phase | s.pos << 3 | s.nk << 7 | s.aux << 11 | s.wmask << 15;
}
LC_HD inline uint32_t lc_popc(uint32_t m) {
  uint32_t c = 0;
  for (; m; m &= m - 1) c++;
  return c;
}
// index (in the sorted key set) of write key number n
LC_HD inline uint32_t lc_nth_bit(uint32_t m, uint32_t n) {
  for (uint32_t k = 0; k < n; k++) m &= m - 1;
  uint32_t j = 0;
  while (j < LC_MAXK - 1 && !((m >> j) & 1u)) j++;
  return j;
}

LC_HD inline uint32_t lc_rnd(uint64_t &r) {  // fastrand
  r = r * 1103515245ull + 12345ull;
  return (uint32_t)(r >> 32);
}
LC_HD inline uint32_t lc_pick(const LcParams &P, uint32_t x) {
  if (P.key_dist == 1) return (uint32_t)zipf_lookup(P.zipf_cdf, P.zipf_n, x);
  return (uint32_t)(((uint64_t)x * P.key_space) >> 32);  // uniform over [0, key_space)
}

// A new transaction (trace_init.sh:12-27): nk = 5 + rnd % 6 distinct keys, drawn until they are distinct; sorted; then
// per key one draw for its kind.  The loops run over fixed indices (an unused slot holds 0xFFFFFFFF and sorts last), so on
// the device the ten keys stay in registers.  Returns the header (phase / mode 0: P_READ = M_ACQ).
template <class S>
LC_HD inline uint32_t lc_new_txn(S &s, const LcParams &P) {
  uint64_t r = s.rng();
  const uint32_t nk = 5 + lc_rnd(r) % 6;
  uint32_t k[LC_MAXK];
#pragma unroll
  for (uint32_t i = 0; i < LC_MAXK; i++) {
    uint32_t v = 0xFFFFFFFFu;
    if (i < nk) {
      bool dup;
      do {
        v = lc_pick(P, lc_rnd(r));
        dup = false;
#pragma unroll
        for (uint32_t j = 0; j < i; j++) dup |= k[j] == v;
      } while (dup);
    }
    k[i] = v;
  }
#pragma unroll
  for (uint32_t a = 0; a < LC_MAXK; a++)  // odd-even transposition sort
#pragma unroll
    for (uint32_t b = a & 1u; b + 1 < LC_MAXK; b += 2) {
      const uint32_t lo = k[b] < k[b + 1] ? k[b] : k[b + 1], hi = k[b] < k[b + 1] ? k[b + 1] : k[b];
      k[b] = lo;
      k[b + 1] = hi;
    }
  uint32_t wm = 0;
#pragma unroll
  for (uint32_t i = 0; i < LC_MAXK; i++)
    if (i < nk && lc_rnd(r) % 100 >= P.read_pct) wm |= 1u << i;
#pragma unroll
  for (uint32_t i = 0; i < LC_MAXK; i++)
    if (i < nk) s.set_key(i, k[i]);
  s.set_rng(r);
  return lc_pack({0u, 0u, nk, 0u, wm});
}

// ---- lock_fasst (client.cc:183-280) ----------------------------------------------------------------------------------
//   READ every key (remember its version)                        :237-245
//   ACQUIRE_LOCK every write key; on REJECT_LOCK ABORT the locks taken so far and restart from the first read  :248-270
//   re-READ every key; a changed version -> ABORT every write key and restart; else COMMIT every write key  :196-235
// the request the worker sends now: its type and the index of its key in the sorted set
LC_HD inline uint32_t lc_fasst_req(uint32_t h, uint8_t *type) {
  const LcState x = lc_unpack(h);
  switch (x.phase) {
    case P_READ: case P_VALIDATE: *type = F_READ; return x.pos;
    case P_ACQ: *type = F_ACQ; break;
    case P_REJ_ABORT: case P_RB_ABORT: *type = F_ABORT; break;
    default: *type = F_COMMIT; break;
  }
  return lc_nth_bit(x.wmask, x.pos);
}

// the worker takes the reply to what lc_fasst_req sent; returns the new header, *ev the LC_EV_* bits
template <class S>
LC_HD inline uint32_t lc_fasst_consume(S &s, uint32_t h, const LcParams &P, uint8_t r_type, uint32_t r_lid, uint32_t r_ver,
                                       uint32_t *ev) {
  uint8_t sent;
  const uint32_t j = lc_fasst_req(h, &sent);
  LcState x = lc_unpack(h);
  const uint32_t nw = lc_popc(x.wmask);
  uint32_t e = r_lid != s.key(j) ? LC_EV_PERR_LID : 0u;  // the asserts of client.cc:205-206,241-242
  bool restart = false, fresh = false;
  switch (x.phase) {
    case P_READ:  // :237-245
      if (r_type != F_GRANT_READ) e |= LC_EV_PERR_TYPE;
      s.set_ver(x.pos, r_ver);
      if (++x.pos == x.nk) { x.pos = 0; x.phase = nw ? P_ACQ : P_VALIDATE; }
      break;
    case P_ACQ:  // :248-270
      if (r_type == F_GRANT_LOCK) {
        if (++x.pos == nw) { x.pos = 0; x.phase = P_VALIDATE; }
      } else if (r_type == F_REJECT_LOCK) {
        e |= LC_EV_REJECT;
        if (x.pos) { x.aux = x.pos; x.pos = 0; x.phase = P_REJ_ABORT; }
        else restart = true;
      } else {
        e |= LC_EV_PERR_TYPE;  // "received wrong packet"
      }
      break;
    case P_REJ_ABORT:
      if (++x.pos == x.aux) restart = true;
      break;
    case P_VALIDATE:  // :196-213
      if (r_ver != s.ver(x.pos)) {
        e |= LC_EV_ROLLBACK;
        if (nw) { x.pos = 0; x.phase = P_RB_ABORT; }
        else restart = true;
      } else if (++x.pos == x.nk) {
        if (nw) { x.pos = 0; x.phase = P_COMMIT; }
        else { e |= LC_EV_COMMIT; fresh = true; }
      }
      break;
    case P_RB_ABORT:  // :215-222
      if (++x.pos == nw) restart = true;
      break;
    default:  // P_COMMIT :224-229
      if (++x.pos == nw) { e |= LC_EV_COMMIT; fresh = true; }
      break;
  }
  *ev = e;
  if (fresh) return lc_new_txn(s, P);
  if (restart) { x.phase = P_READ; x.pos = 0; }
  return lc_pack(x);
}

// ---- lock_2pl (client.cc:167-240, as dint_amd/driver.py::TplClient) ------------------------------------------------------
//   ACQUIRE the locks in ascending order; on REJECT with locks held RELEASE them in acquisition order, then try the same
//   transaction again; on REJECT with nothing held send the same ACQUIRE again; once every lock is held RELEASE them in
//   reverse order: the transaction has committed.
// the request the worker sends now: its action and lock type; returns the index of its key
LC_HD inline uint32_t lc_tpl_req(uint32_t h, uint8_t *action, uint8_t *type) {
  const LcState x = lc_unpack(h);
  *action = x.phase == M_ACQ ? L_ACQUIRE : L_RELEASE;
  *type = (uint8_t)((x.wmask >> x.pos) & 1u);
  return x.pos;
}

template <class S>
LC_HD inline uint32_t lc_tpl_consume(S &s, uint32_t h, const LcParams &P, uint8_t r_action, uint32_t *ev) {
  LcState x = lc_unpack(h);
  uint32_t e = 0;
  if (x.phase == M_ACQ) {
    if (r_action == L_GRANT) {
      x.aux++;
      if (++x.pos == x.nk) { x.phase = M_REL; x.pos = x.nk - 1; }
    } else if (r_action == L_REJECT) {
      e |= LC_EV_REJECT;
      if (x.aux) { x.phase = M_ROLL; x.pos = 0; }
    } else {
      e |= LC_EV_PERR_TYPE;  // (the reference asserts kRetry; the same ACQUIRE goes out again)
    }
  } else if (x.phase == M_ROLL) {
    if (r_action != L_RELEASE_ACK) e |= LC_EV_PERR_TYPE;
    if (++x.pos == x.aux) { x.phase = M_ACQ; x.pos = 0; x.aux = 0; }
  } else {
    if (r_action != L_RELEASE_ACK) e |= LC_EV_PERR_TYPE;
    if (x.pos == 0) {
      *ev = e | LC_EV_COMMIT;
      return lc_new_txn(s, P);
    }
    x.pos--;
  }
  *ev = e;
  return lc_pack(x);
}

// ---- host storage of one worker ---------------------------------------------------------------------------------------
struct LcWorker {
  uint64_t r;
  uint32_t hdr;
  uint32_t keys[LC_MAXK], vers[LC_MAXK];
  uint64_t rng() const { return r; }
  void set_rng(uint64_t v) { r = v; }
  uint32_t key(uint32_t j) const { return keys[j]; }
  void set_key(uint32_t j, uint32_t v) { keys[j] = v; }
  uint32_t ver(uint32_t j) const { return vers[j]; }
  void set_ver(uint32_t j, uint32_t v) { vers[j] = v; }
};
