/*
 * ref_client.cc -- runs ONE client of the reference (the UNMODIFIED <wl>/caladan/client_udp_shard.cc, named by
 * -DCLIENT_SRC and found through -I$(REF)/<wl>/caladan) against three CPU oracle shard servers and records, per shard,
 * the requests it sent and the replies it got.  TEST INFRASTRUCTURE ONLY (the pin of the transaction
 * handlers).  See stub/caladan_stub.h for how the Caladan runtime is stood in for.
 *
 * So that the abort paths run too, every 7th lock request is answered REJECT by this harness itself, as if another
 * client held the lock (the server is not touched; the reference client then releases what it holds and gives up the
 * transaction -- tatp/caladan/client_udp_shard.cc:400-420).
 *
 * usage: ref_client_<wl> <worker gid> <messages> <out prefix>     -> <prefix>.s{0,1,2}.req / .rep (packed wire structs)
 *        ref_client_<wl> <first gid> <messages> <out prefix> <n>  -> <prefix>.<gid>.s{0,1,2}.req / .rep for n consecutive
 *            gids, one client after the other (<messages> each) against the SAME three servers, which are populated
 *            once: a client whose budget ran out inside a transaction leaves its locks behind, and the clients after it
 *            are refused by the server where they meet one (tests/golden/make_golden_clients_block.py)
 */
#define main ref_client_main
#include CLIENT_SRC
#undef main

extern "C" {
#include "dint_oracle.h"
}

static void *g_shard[3];
static FILE *g_req[3], *g_rep[3];
static uint64_t g_budget, g_sent, g_locks, g_refused;

void ref_client_server(uint32_t ip, void *msg, size_t len) {
  int s = -1;
  for (int i = 0; i < 3; i++)
    if (servaddr[i].ip == ip) s = i;
  if (s < 0 || len != sizeof(message)) panic("message of %zu bytes to an unknown server", len);
  if (g_sent >= g_budget) throw ref_client_stop();
  g_sent++;
  fwrite(msg, 1, len, g_req[s]);
  message *m = (message *)msg;
  bool refused = false;
#ifdef REF_SMALLBANK
  if (m->type == PktType::kAcquireShared || m->type == PktType::kAcquireExclusive) {
    if (g_locks++ % 7 == 3) { m->type = m->type == PktType::kAcquireShared ? PktType::kRejectShared : PktType::kRejectExclusive; refused = true; }
  }
  g_refused += refused;
  if (!refused) orc_sb_replay((orc_sb *)g_shard[s], msg, 1);
#else
  if (m->type == PktType::kAcquireLock) {
    if (g_locks++ % 7 == 3) { m->type = PktType::kRejectLock; refused = true; }
  }
  g_refused += refused;
  if (!refused) orc_tatp_replay((orc_tatp *)g_shard[s], msg, 1);
#endif
  fwrite(msg, 1, len, g_rep[s]);
}

static int open_out(const char *prefix, int gid, bool block) {
  for (int s = 0; s < 3; s++) {
    char stem[4096], p[4200];
    if (block) snprintf(stem, sizeof stem, "%s.%d", prefix, gid);
    else snprintf(stem, sizeof stem, "%s", prefix);
    snprintf(p, sizeof p, "%s.s%d.req", stem, s);
    g_req[s] = fopen(p, "wb");
    snprintf(p, sizeof p, "%s.s%d.rep", stem, s);
    g_rep[s] = fopen(p, "wb");
    if (!g_req[s] || !g_rep[s]) { perror("output"); return 2; }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4 && argc != 5) { fprintf(stderr, "usage: %s <worker gid> <messages> <out prefix> [<clients>]\n", argv[0]); return 2; }
  const int gid0 = atoi(argv[1]), n = argc == 5 ? atoi(argv[4]) : 1;
  g_budget = strtoull(argv[2], nullptr, 10);
  if (n < 1) { fprintf(stderr, "<clients> must be positive\n"); return 2; }
  for (int s = 0; s < 3; s++) {
#ifdef REF_SMALLBANK
    g_shard[s] = orc_sb_create(kAccountNum, 1000000, kAccountNum);
#else
    g_shard[s] = orc_tatp_create(kSubscriberNum, 1000000, kSubscriberNum);
#endif
    servaddr[s].ip = MAKE_IP_ADDR(10, 10, 1, 1 + s);
    servaddr[s].port = kFasstPort;
  }
  /* what the reference's main() sets up before it starts the runtime (client_udp_shard.cc:1202-1236) */
  machine_id = 0;
  threads = 1 << 30;  /* wrkr_lid = wrkr_gid % threads = gid; the statistics arrays below are never indexed (stat_started stays false) */
  mode = "expr";
  net_intv = 0;
  CreateWorkgenArr();
#ifndef REF_SMALLBANK
  create_map1000();
#endif
  for (int gid = gid0; gid < gid0 + n; gid++) {
    if (open_out(argv[3], gid, argc == 5)) return 2;
    g_sent = g_refused = 0;  /* (g_locks runs on: every 7th lock request of the whole run) */
    try {
      ClientLoop(gid);
    } catch (const ref_client_stop &) {
    }
    for (int s = 0; s < 3; s++) { fclose(g_req[s]); fclose(g_rep[s]); }
    printf("{\"gid\": %d, \"messages\": %llu, \"locks_refused\": %llu}\n", gid, (unsigned long long)g_sent,
           (unsigned long long)g_refused);
  }
  return 0;
}
