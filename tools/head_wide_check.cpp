// head_wide_check.cpp — the host's decision for the wide head ladder
// (csrc/prove_plan.h: head_wide_decide / head_wide_observe) on a machine
// without a GPU: replays the proofs of one head column given on the command
// line and prints, per proof, the decision and the ladder then in place.
//   head_wide_check <proof>...
//   <proof> = epoch:cap:lo:hi:mlo:mhi:delta:wide:fb_start:fb_span
// (what the proof runs under, and what it reports when it completes; wide,
// fb_start and fb_span are what the device would count, given by the caller)
#include <stdio.h>
#include <stdlib.h>

#include "../streaming-zero-knowledge-proofs_amd/csrc/prove_plan.h"

int main(int argc, char** argv) {
  using namespace sezkp;
  HeadWideCol col;
  printf("[");
  for (int i = 1; i < argc; i++) {
    long long v[10];
    char* p = argv[i];
    for (int j = 0; j < 10; j++) {
      char* end = nullptr;
      v[j] = strtoll(p, &end, 10);
      if (end == p || (j < 9 ? *end != ':' : *end != 0)) {
        fprintf(stderr, "bad proof '%s'\n", argv[i]);
        return 2;
      }
      p = end + 1;
    }
    const uint64_t epoch = (uint64_t)v[0];
    const HeadWideDecision d = head_wide_decide(col, epoch, (uint64_t)v[1]);
    const bool in_place = col.epoch == epoch && epoch != 0;
    printf("%s{\"use\": %d, \"build\": %d, \"l3\": %llu, \"low\": %llu, \"in_place\": %d, \"olo\": %lld, \"span\": %u, "
           "\"dmin\": %lld, \"dR\": %u",
           i > 1 ? ", " : "", (int)d.use, (int)d.build, (unsigned long long)d.l3_entries,
           (unsigned long long)d.low_entries, (int)in_place, (long long)col.olo, col.span, (long long)col.dmin, col.dR);
    HeadWideObs o;
    o.lo = v[2];
    o.hi = v[3];
    o.mlo = v[4];
    o.mhi = v[5];
    o.delta = (uint32_t)v[6];
    o.wide = (uint32_t)v[7];
    o.fb_start = (uint32_t)v[8];
    o.fb_span = (uint32_t)v[9];
    head_wide_observe(col, epoch, o);
    printf(", \"respan\": %d}", (int)col.respan);
  }
  printf("]\n");
  return 0;
}
