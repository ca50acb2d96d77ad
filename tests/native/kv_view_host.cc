// The host build of the HBM table layout (kv_core_host.cc, included as it is) with what the table verify's CPU test needs on
// top: the table described as a dint_tables_view's pointers and control block, a reclaim's head words taken back, an insert
// that names its free list, and a leak made by hand.  TEST TOOLING ONLY -- built by tests/test_state_verify_host.py with g++.
#include "kv_core_host.cc"

extern "C" {

// ctl = 1600 bytes in the engine's layout: pool_top at 0, free_head[64] at 64, pend_head[2][64] behind it (the host build has
// one pend set: set 0)
void kvh_view_fill(kvh *h, uint8_t *ctl, void **entries, void **pool_next) {
  memset(ctl, 0, 64 + 24 * KV_NLISTS);
  memcpy(ctl, &h->pool_top, 4);
  memcpy(ctl + 64, h->free_head, sizeof h->free_head);
  memcpy(ctl + 64 + 8 * KV_NLISTS, h->pend_head, sizeof h->pend_head);
  *entries = h->t.entries;
  *pool_next = h->t.pool_next;
}
// after a reclaim over the view: the free lists' head words (the only control words a reclaim writes)
void kvh_view_store(kvh *h, const uint8_t *ctl) { memcpy(h->free_head, ctl + 64, sizeof h->free_head); }
int kvh_insert_list(kvh *h, uint64_t bucket, uint64_t key, const uint8_t *val, uint32_t ver, uint32_t lst) {
  const kv_hdr H = *kv_entry_hdr(h->t, bucket, KV_INLINE);
  return kv_apply<kv_host_mem>(h->t, bucket, H, KV_ACT_INS, key, (uint8_t *)val, ver, lst).ok ? 0 : 1;
}
// n entries handed out and never linked, each with a stale valid byte and link; returns how many the pool gave
uint32_t kvh_leak(kvh *h, uint32_t n) {
  uint32_t got = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t link = kv_pool_alloc<kv_host_mem>(h->t, 0);
    if (link == KV_NULL) break;
    kv_hdr *e = kv_entry_hdr(h->t, 0, link);
    e->validw = 1;
    e->next = 2;
    got++;
  }
  return got;
}
}
