// tpl_client.cc -- the lock_2pl load generator (the CALLER of the lock_2pl path), restated as an epoch-synchronous
// closed loop.  Plain host C++.
//
// Reference: lock_2pl/caladan/client.cc:167-240 (ClientLoop) over traces made by lock_2pl/caladan/trace_init.sh:6-27 --
// per transaction 5..10 distinct locks in ascending order, each exclusive with probability 1 - r_prop (r_prop = 0.8).  One
// uthread = one worker with ONE request outstanding: ACQUIRE the locks one by one; a REJECT releases what the
// transaction holds (in acquisition order) and starts it again; once all are held, RELEASE them in reverse order.  The
// transactions are drawn exactly as the lock_fasst client draws them (lock_clients.h: the reference's own LCG seeded
// 0xdeadbeef + worker, keys uniform or Zipf(theta)) -- unlike dint_amd/driver.py::TplClient, whose numpy draws no C or
// HIP code can reproduce; the state machine is TplClient's.
#include <string.h>

#include <new>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "lock_clients.h"

int dint_lock_client_params(const dint_fasst_client_config *cfg, LcParams *P, ZipfTable *zipf);  // fasst_client.cc

struct dint_tpl_client {
  dint_fasst_client_config cfg{};
  dint_tpl_client_stats st{};
  std::vector<LcWorker> w;
  std::vector<TplMsg> out;
  ZipfTable zipf;
  LcParams P{};
  bool awaiting = false;
};

extern "C" {

int dint_tpl_client_create(const dint_fasst_client_config *cfg, dint_tpl_client_t **out) {
  if (!cfg || !out) return DINT_EINVAL;
  try {
    dint_tpl_client *c = new dint_tpl_client();
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

void dint_tpl_client_destroy(dint_tpl_client_t *c) { delete c; }

// one request per worker, in worker order; returns the batch (n_workers 6-byte messages, valid until the next call)
const void *dint_tpl_client_next(dint_tpl_client_t *c) {
  if (!c || c->awaiting) return nullptr;
  for (size_t i = 0; i < c->w.size(); i++) {
    const LcWorker &x = c->w[i];
    uint8_t action, type;
    const uint32_t j = lc_tpl_req(x.hdr, &action, &type);
    c->out[i] = TplMsg{action, x.keys[j], type};
  }
  c->st.requests += c->w.size();
  c->st.epochs++;
  c->awaiting = true;
  return c->out.data();
}

int dint_tpl_client_consume(dint_tpl_client_t *c, const void *replies) {
  if (!c || !replies) return DINT_EINVAL;
  if (!c->awaiting) return DINT_ESTATE;
  const TplMsg *rep = (const TplMsg *)replies;
  for (size_t i = 0; i < c->w.size(); i++) {
    LcWorker &x = c->w[i];
    uint32_t ev;
    x.hdr = lc_tpl_consume(x, x.hdr, c->P, rep[i].action, &ev);
    c->st.committed += (ev & LC_EV_COMMIT) != 0;
    c->st.rejects += (ev & LC_EV_REJECT) != 0;
    c->st.protocol_errors += (ev & LC_EV_PERR_TYPE) != 0;
  }
  c->awaiting = false;
  return 0;
}

// the transaction `worker` is running: its locks in ascending order and their types (1 = exclusive) -- one transaction
// of lock_2pl/caladan/trace_init.sh's trace files (tests/golden/make_golden_clients_micro_lcg.py)
int dint_tpl_client_peek(const dint_tpl_client_t *c, uint32_t worker, uint32_t *lids, uint8_t *types, uint32_t *n_locks) {
  if (!c || !lids || !types || !n_locks || worker >= c->w.size()) return DINT_EINVAL;
  const LcWorker &x = c->w[worker];
  const LcState s = lc_unpack(x.hdr);
  *n_locks = s.nk;
  memcpy(lids, x.keys, sizeof(uint32_t) * s.nk);
  for (uint32_t j = 0; j < s.nk; j++) types[j] = (uint8_t)((s.wmask >> j) & 1u);
  return 0;
}

int dint_tpl_client_get_stats(const dint_tpl_client_t *c, dint_tpl_client_stats *out) {
  if (!c || !out) return DINT_EINVAL;
  *out = c->st;
  return 0;
}

}  // extern "C"
