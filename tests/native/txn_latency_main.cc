// txn_latency_main.cc -- the round-trip count of a client header at its ceiling (dint_amd/csrc/txn_latency.h), through the
// host driver of dint_amd/csrc/txn_driver.cc, as a program of its own for AddressSanitizer / UBSan
// (tests/test_txn_latency_host.py builds and runs it).
//
// A client's transaction is under way, its round-trip byte is set to 254, and the transaction goes on through at least two
// more phases against a stand-in server that grants everything: the byte reaches 255 and stays, the transaction is counted in
// bin 31 with rt_sum = rt_max = 255, and the transaction after it counts from zero again.
#include <stdio.h>

#include "../../dint_amd/csrc/txn_driver.cc"

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) { failures++; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

static void grant(TatpMsg &m) { m.type = m.type == T_READ ? T_GRANT_READ : m.type == T_ACQ ? T_GRANT_LOCK : m.type; }
static void grant(SbMsg &m) { m.type = m.type == S_ACQ_SH ? S_GRANT_SH : m.type == S_ACQ_EX ? S_GRANT_EX : m.type; }

template <class T>
static uint8_t &rt_byte(typename T::Client &c);
template <> uint8_t &rt_byte<TatpTraits>(TatpClient &c) { return c.pad_[0]; }
template <> uint8_t &rt_byte<SbTraits>(SbClient &c) { return c.pad0; }

// one epoch: the requests answered in place by a server that grants every read and lock
template <class T>
static void epoch(dint_driver_t *d) {
  typedef typename T::Msg Msg;
  uint32_t cnt[DINT_N_SHARDS];
  CHECK(dint_driver_next(d, cnt) == 0);
  std::vector<Msg> rep[DINT_N_SHARDS];
  const void *ptr[DINT_N_SHARDS];
  for (uint32_t s = 0; s < DINT_N_SHARDS; s++) {
    const Msg *q = (const Msg *)dint_driver_batch(d, s);
    rep[s].assign(q, q + cnt[s]);  // exactly the batch's size: a read past it is the sanitizer's
    for (auto &m : rep[s]) grant(m);
    ptr[s] = rep[s].data();
  }
  CHECK(dint_driver_consume(d, ptr) == 0);
}

template <class T>
static void run(uint32_t workload, uint8_t want_txn, uint32_t min_phases) {
  for (uint32_t first = 0; first < 1000; first++) {  // a client whose first transaction is the long one
    dint_driver_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.workload = workload; cfg.n_clients = 1; cfg.n_rows = 1000; cfg.first_client = first;
    dint_driver_t *d = nullptr;
    CHECK(dint_driver_create(&cfg, &d) == 0 && d);
    auto *h = static_cast<HostDriver<T> *>(d);
    epoch<T>(d);
    if (h->cl[0].txn != want_txn) { dint_driver_destroy(d); continue; }
    CHECK(rt_byte<T>(h->cl[0]) == 1);
    rt_byte<T>(h->cl[0]) = 254;
    dint_driver_stats st;
    uint32_t phases = 0;
    do {
      epoch<T>(d);
      phases++;
      CHECK(dint_driver_get_stats(d, &st) == 0);
      if (!st.txns) CHECK(rt_byte<T>(h->cl[0]) == 255);  // 254 -> 255 -> 255: no wrap
    } while (!st.txns && phases < 64);
    CHECK(st.txns == 1 && st.committed == 1 && phases >= min_phases);
    dint_driver_latency L;
    CHECK(dint_driver_get_latency(d, &L) == 0);
    uint64_t all = 0;
    for (int t = 0; t < 8; t++)
      for (int r = 0; r < DINT_LAT_RT_BINS; r++) all += L.round_trips[t][r] + L.aborted_round_trips[t][r];
    CHECK(all == 1 && L.round_trips[want_txn][DINT_LAT_RT_BINS - 1] == 1);
    CHECK(L.rt_sum[want_txn] == 255 && L.rt_max[want_txn] == 255);
    CHECK(rt_byte<T>(h->cl[0]) == 1);  // the next transaction began in the phase that finished this one
    CHECK(L.epochs == st.epochs && L.tick_khz == 0 && L.tick_sum[want_txn] == 0);
    // the transaction after it: counted from zero
    const uint8_t next_txn = h->cl[0].txn;
    uint32_t more = 0;
    do {
      epoch<T>(d);
      more++;
      CHECK(dint_driver_get_stats(d, &st) == 0);
    } while (st.txns < 2 && more < 64);
    CHECK(st.txns == 2 && dint_driver_get_latency(d, &L) == 0);
    const uint64_t(*hist)[DINT_LAT_RT_BINS] = st.committed == 2 ? L.round_trips : L.aborted_round_trips;
    CHECK(more < DINT_LAT_RT_BINS - 1 && hist[next_txn][more] == 1);
    CHECK(L.rt_max[want_txn] == 255);
    dint_driver_destroy(d);
    return;
  }
  CHECK(!"no client drew the transaction");
}

int main() {
  // the tick bin rule at its ends, through the exported functions
  CHECK(dint_latency_tick_bin_host(0) == 0 && dint_latency_tick_bin_host(15) == 15 && dint_latency_tick_bin_host(16) == 16);
  CHECK(dint_latency_tick_bin_host(~0ull) == DINT_LAT_TICK_BINS - 1 && dint_latency_tick_bin_host(1ull << 63) == DINT_LAT_TICK_BINS - 1);
  CHECK(dint_latency_tick_lo_host(DINT_LAT_TICK_BINS) == 1ull << 32);
  for (uint32_t b = 0; b < DINT_LAT_TICK_BINS; b++) CHECK(dint_latency_tick_bin_host(dint_latency_tick_lo_host(b)) == b);
  run<TatpTraits>(DINT_WL_TATP, TT_UPD_LOC, 5);          // UpdateLocation: 6 phases, finished in the 7th
  run<SbTraits>(DINT_WL_SMALLBANK, ST_DEPOSIT_CHECKING, 4);  // DepositChecking: lock, log, backup, primary, release
  printf("%d failures\n", failures);
  return failures != 0;
}
