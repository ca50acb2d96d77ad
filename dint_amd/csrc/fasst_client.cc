// fasst_client.cc -- the lock_fasst load generator (the CALLER of the lock_fasst path), restated as an
// epoch-synchronous closed loop.  Plain host C++.
//
// Reference: lock_fasst/caladan/client.cc:183-280 (ClientLoop) over traces made by lock_fasst/caladan/trace_init.sh
// :6-27 -- per transaction 5..10 distinct keys, sorted; every key is read; each key is also written with probability
// 1 - r_prop (r_prop = 0.8).  One uthread = one worker with ONE request outstanding:
//   READ every read key (remember its version)               client.cc:237-245
//   ACQUIRE_LOCK every write key; on REJECT_LOCK send ABORT for the locks taken so far and restart the
//   transaction from its first read                          :248-270
//   when the transaction's last request is done: re-READ every read key; a changed version -> ABORT every write
//   key and restart the transaction; else COMMIT every write key   :196-235
// W workers run in lock step: one EPOCH = every worker's next request, in worker order (models W concurrent
// clients, so REJECTs, roll-backs and aborts really happen); the epochs laid end to end are the request trace.
// The reference's traces are unseeded Python `random.sample` output, so no fixed trace ships with it:
// here every worker draws its transactions from the reference's own LCG (`fastrand`, tatp/caladan/tatp.h:31-34) seeded
// 0xdeadbeef + worker, keys uniform (the reference) or Zipf(theta) over the key space.  A worker never wraps around
// to its first transaction (the reference replays its 20,000-transaction file in a loop; 24M requests over 4096
// workers are ~320 transactions each).
#include <string.h>

#include <new>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "lock_clients.h"

// The worker state machine lives in lock_clients.h (shared with the GPU-resident client, k_lock_client.hip); this file
// is its host loop over the workers.
struct dint_fasst_client {
  dint_fasst_client_config cfg{};
  dint_fasst_client_stats st{};
  std::vector<LcWorker> w;
  std::vector<FasstMsg> out;
  ZipfTable zipf;
  LcParams P{};
  bool awaiting = false;
};

// the config check and the key distribution, shared with the 2PL host client (tpl_client.cc) and the GPU client
int dint_lock_client_params(const dint_fasst_client_config *cfg, LcParams *P, ZipfTable *zipf) {
  if (!cfg || cfg->n_workers == 0 || cfg->key_space < 16 || cfg->read_pct > 100 || cfg->key_dist > 1) return DINT_EINVAL;
  if (cfg->key_dist == 1 && !(cfg->zipf_theta > 0 && cfg->zipf_theta < 1)) return DINT_EINVAL;
  *P = LcParams{cfg->key_space, cfg->read_pct, cfg->key_dist, 0, cfg->key_space, nullptr};
  if (cfg->key_dist == 1) {
    zipf->init(cfg->key_space, cfg->zipf_theta);
    P->zipf_cdf = zipf->cdf.data();
  }
  return 0;
}

extern "C" {

int dint_fasst_client_create(const dint_fasst_client_config *cfg, dint_fasst_client_t **out) {
  if (!cfg || !out) return DINT_EINVAL;
  try {
    dint_fasst_client *c = new dint_fasst_client();
    if (int rc = dint_lock_client_params(cfg, &c->P, &c->zipf)) {
      delete c;
      return rc;
    }
    c->cfg = *cfg;
    c->w.resize(cfg->n_workers);
    c->out.resize(cfg->n_workers);
    for (uint32_t i = 0; i < cfg->n_workers; i++) {
      c->w[i].r = 0xdeadbeefull + cfg->first_worker + i;
      c->w[i].hdr = lc_new_txn(c->w[i], c->P);
    }
    *out = c;
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
  return 0;
}

void dint_fasst_client_destroy(dint_fasst_client_t *c) { delete c; }

// one request per worker, in worker order; returns the batch (n_workers 9-byte messages, valid until the next call)
const void *dint_fasst_client_next(dint_fasst_client_t *c) {
  if (!c || c->awaiting) return nullptr;
  for (size_t i = 0; i < c->w.size(); i++) {
    const LcWorker &x = c->w[i];
    uint8_t type;
    const uint32_t j = lc_fasst_req(x.hdr, &type);
    c->out[i] = FasstMsg{type, x.keys[j], 0};
  }
  c->st.requests += c->w.size();
  c->st.epochs++;
  c->awaiting = true;
  return c->out.data();
}

int dint_fasst_client_consume(dint_fasst_client_t *c, const void *replies) {
  if (!c || !replies) return DINT_EINVAL;
  if (!c->awaiting) return DINT_ESTATE;
  const FasstMsg *rep = (const FasstMsg *)replies;
  for (size_t i = 0; i < c->w.size(); i++) {
    LcWorker &x = c->w[i];
    const FasstMsg r = rep[i];
    uint32_t ev;
    x.hdr = lc_fasst_consume(x, x.hdr, c->P, r.type, r.lid, r.ver, &ev);
    c->st.committed += (ev & LC_EV_COMMIT) != 0;
    c->st.rejects += (ev & LC_EV_REJECT) != 0;
    c->st.rollbacks += (ev & LC_EV_ROLLBACK) != 0;
    c->st.protocol_errors += ((ev & LC_EV_PERR_LID) != 0) + ((ev & LC_EV_PERR_TYPE) != 0);
  }
  c->awaiting = false;
  return 0;
}

// the transaction worker `worker` is running: its sorted read set (all keys) and its write set, as one transaction of the
// reference's trace files lists them (trace_init.sh:20-27).  For the pin against the unmodified reference client, which
// reads its transactions from such a file (tests/golden/make_golden_clients_micro.py).
int dint_fasst_client_peek(const dint_fasst_client_t *c, uint32_t worker, uint32_t *keys, uint32_t *n_keys, uint32_t *wkeys,
                           uint32_t *n_wkeys) {
  if (!c || !keys || !n_keys || !wkeys || !n_wkeys || worker >= c->w.size()) return DINT_EINVAL;
  const LcWorker &x = c->w[worker];
  const LcState s = lc_unpack(x.hdr);
  *n_keys = s.nk;
  *n_wkeys = 0;
  memcpy(keys, x.keys, sizeof(uint32_t) * s.nk);
  for (uint32_t j = 0; j < s.nk; j++)
    if ((s.wmask >> j) & 1u) wkeys[(*n_wkeys)++] = x.keys[j];
  return 0;
}

int dint_fasst_client_get_stats(const dint_fasst_client_t *c, dint_fasst_client_stats *out) {
  if (!c || !out) return DINT_EINVAL;
  *out = c->st;
  return 0;
}

}  // extern "C"
