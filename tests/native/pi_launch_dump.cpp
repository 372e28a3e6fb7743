// Test helper (host only): how plan creation (tapir_amd/csrc/site_launch_plan.hpp) will run the PI partial sums of a batch, and
// the workspace it lays out for it.  Records on stdin, one per line:
//   shape <ntaxa> <nwords> <stack_depth> <T> <n_i>
//   cus <CU count>
//   loci <count> <columns each>            (may repeat: the loci are appended)
//   knob <TPHIP_...> <text>                (the text an environment variable would hold)
// Every occupancy query answers 8 workgroups per CU.  Prints "name value" lines: pi_split, compact_chunked, n_pi_chunks and
// the workspace offsets.
#include <cstdio>
#include <utility>
#include <vector>
#include "site_launch_plan.hpp"

using namespace tphip;

int main() {
    SiteShape shape;
    PlanKnobs knobs;
    int cus = 0;
    std::vector<int64_t> offsets(1, 0);
    char line[512], name[128], text[256];
    while (fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0;
        if (sscanf(line, "shape %d %d %d %d %d", &shape.ntaxa, &shape.nwords, &shape.stack_depth, &shape.T, &shape.n_i) == 5) continue;
        if (sscanf(line, "cus %d", &cus) == 1) continue;
        if (sscanf(line, "loci %lld %lld", &a, &b) == 2) {
            for (long long l = 0; l < a; ++l) offsets.push_back(offsets.back() + b);
            continue;
        }
        text[0] = 0;
        if (sscanf(line, "knob %127s %255s", name, text) >= 1) {
            if (!set_plan_knob(&knobs, name, text)) { fprintf(stderr, "no knob %s\n", name); return 2; }
            continue;
        }
        if (line[0] != '\n') { fprintf(stderr, "bad line: %s", line); return 2; }
    }
    shape.nloci = (int64_t)offsets.size() - 1;
    shape.ncols = offsets.back();
    for (size_t l = 0; l + 1 < offsets.size(); ++l) shape.max_locus_cols = std::max(shape.max_locus_cols, offsets[l + 1] - offsets[l]);
    if (cus < 1 || shape.nloci < 1) { fprintf(stderr, "need cus and loci\n"); return 2; }

    const SiteLaunch s = decide_site_launch(shape, cus, knobs, [](int, size_t) { return 8; });
    const ChunkTables t = build_chunk_tables(offsets.data(), shape.nloci, s.chunk_cols);
    const WorkspaceLayout w = layout_workspace(shape, s, (int64_t)t.pi_chunk_locus.size());
    printf("pi_split %d\ncompact_chunked %d\nmax_locus_cols %lld\nn_pi_chunks %zu\n", s.pi_split, s.compact_chunked,
           (long long)shape.max_locus_cols, t.pi_chunk_locus.size());
    const std::pair<const char*, size_t> regions[] = {
        {"work_cols", w.work_cols}, {"work_cols2", w.work_cols2}, {"work_count", w.work_count}, {"work_prefix", w.work_prefix},
        {"slice_prefix", w.slice_prefix}, {"work_class", w.work_class}, {"work_wprefix", w.work_wprefix}, {"part_prefix", w.part_prefix},
        {"part_start", w.part_start}, {"chunk_cnt", w.chunk_cnt}, {"partial", w.partial}, {"packed", w.packed}, {"hash", w.hash},
        {"dup_of", w.dup_of}, {"tab_key", w.tab_key}, {"tab_val", w.tab_val}, {"dedup_on", w.dedup_on}, {"spill", w.spill},
        {"total", w.total}};
    for (const auto& r : regions) printf("ws.%s %zu\n", r.first, r.second);
    return 0;
}
