// The host build of the HBM table layout with the view of kv_view_host.cc (included as it is) and what the compaction's CPU
// test needs on top: ALL control words taken back after a compaction over the view -- pool_top, the free lists' head words and
// the one pend set's.  TEST TOOLING ONLY -- built by tests/test_state_compact_host.py with g++.
#include "kv_view_host.cc"

extern "C" {
void kvh_ctl_store(kvh *h, const uint8_t *ctl) {
  memcpy(&h->pool_top, ctl, 4);
  memcpy(h->free_head, ctl + 64, sizeof h->free_head);
  memcpy(h->pend_head, ctl + 64 + 8 * KV_NLISTS, sizeof h->pend_head);
}
}
