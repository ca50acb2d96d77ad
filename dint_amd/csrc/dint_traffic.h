// dint_traffic.h -- the traffic report's launchers (k_traffic.hip) as engine.hip calls them; the rule is traffic_report.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "traffic_report.h"

// a call's own device memory: one arena sized by n (the arrays of k_traffic.hip's stages, carved by dint_traffic_run), the result
// words, the decode stage's partials and the two lists.  dint_traffic_run allocates what is missing or too small; the caller frees
// it (dint_traffic_report: before it returns -- the engine keeps none of it)
struct dint_traffic_scratch {
  void *arena = nullptr;
  size_t arena_bytes = 0;
  unsigned long long *words = nullptr;
  uint32_t *part = nullptr;
  dint_traffic_key *top = nullptr;  // [2][DINT_TRAFFIC_MAX_TOP]
};
// the geometry of an engine created with (workload, n_slots, n_rows, flags): the bucket counts come from dint_kv_hash_sizes, which
// dint_kv_create builds the tables with.  false: a workload without keys
bool dint_traffic_geom(uint32_t workload, uint64_t n_slots, uint64_t n_rows, uint32_t flags, tr_geom *g);
// the whole report of a checked call (n <= DINT_TRAFFIC_MAX_N, top_k <= DINT_TRAFFIC_MAX_TOP) on `st`: three synchronisations.
// out and the lists are written only by a call that returns 0; DINT_ENOMEM / DINT_EHIP otherwise
int dint_traffic_run(const tr_geom &g, dint_traffic_scratch &s, const void *d_req, const void *d_rep, uint64_t n, uint32_t top_k, hipStream_t st,
                     struct dint_traffic_report *out, dint_traffic_key *by_requests, dint_traffic_key *by_rejects);
void dint_traffic_free(dint_traffic_scratch &s);
void dint_set_last_error(const char *msg);  // engine.hip
