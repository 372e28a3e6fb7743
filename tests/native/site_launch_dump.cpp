// Test helper (host only): the launch decisions of plan creation (tapir_amd/csrc/site_launch_plan.hpp) for a shape, knobs
// and an occupancy table read from stdin, one record per line:
//   shape <ntaxa> <nwords> <stack_depth> <model> <ncat> <start_rule> <pattern_dedup> <T> <n_i>
//   cus <CU count>
//   loci <count> <columns each>            (may repeat: the loci are appended)
//   knob <TPHIP_...> <text>                (the text an environment variable would hold)
//   occ <variant> <lds_bytes> <resident workgroups per CU>
// Prints the SiteLaunch fields, the occupancy queries made (in order), the chunk-table sizes, the workspace offsets, the
// launch grid and the launch arguments (site_kernel_args, as "args.<name>") as "name value" lines.  An occupancy query that the table does not hold answers 0, as a failed one does.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "site_launch_plan.hpp"

using namespace tphip;

int main() {
    SiteShape shape;
    PlanKnobs knobs;
    int cus = 0;
    std::vector<int64_t> offsets(1, 0);
    std::map<std::pair<int, size_t>, int> table;
    char line[512], name[128], text[256];
    while (fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0;
        int v = 0, n = 0;
        if (sscanf(line, "shape %d %d %d %d %d %d %d %d %d", &shape.ntaxa, &shape.nwords, &shape.stack_depth, &shape.model, &shape.ncat,
                   &shape.start_rule, &shape.pattern_dedup, &shape.T, &shape.n_i) == 9) continue;
        if (sscanf(line, "cus %d", &cus) == 1) continue;
        if (sscanf(line, "loci %lld %lld", &a, &b) == 2) {
            for (long long l = 0; l < a; ++l) offsets.push_back(offsets.back() + b);
            continue;
        }
        if (sscanf(line, "occ %d %lld %d", &v, &a, &n) == 3) { table[{v, (size_t)a}] = n; continue; }
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

    std::string queries;
    const SiteLaunch s = decide_site_launch(shape, cus, knobs, [&](int variant, size_t lds) {
        queries += " " + std::to_string(variant) + ":" + std::to_string(lds);
        const auto it = table.find({variant, lds});
        return it == table.end() ? 0 : it->second;
    });
    const ChunkTables t = build_chunk_tables(offsets.data(), shape.nloci, s.chunk_cols);
    const WorkspaceLayout w = layout_workspace(shape, s, (int64_t)t.pi_chunk_locus.size());

    printf("start_rule %d\ndedup_mode %d\nchunk_cols %d\nwaves %d\npersistent %d\nmixed %d\n", s.start_rule, s.dedup_mode, s.chunk_cols,
           s.waves, s.persistent, s.mixed);
    printf("mixed_few_waves %d\nmixed_switch_cols %lld\ngrid_mult %d\nlds_depth %d\nfirst_fraction %.17g\ntail_order %d\n", s.mixed_few_waves,
           (long long)s.mixed_switch_cols, s.grid_mult, s.lds_depth, s.first_fraction, s.tail_order);
    printf("share_work %d\nreserve_q %d\nw_slow %d\nw_easy %d\ncompact_chunked %d\nhost_split %d\n", s.share_work, s.reserve_q, s.w_slow,
           s.w_easy, s.compact_chunked, host_split_groups(knobs));
    printf("queries%s\n", queries.c_str());
    printf("n_site_chunks %zu\nn_pi_chunks %zu\n", t.site_chunk_locus.size(), t.pi_chunk_locus.size());
    // the tables themselves: sizes agree, every chunk lies inside its locus, the PI chunks of a locus are consecutive
    bool ok = t.site_chunk_index.size() == t.site_chunk_locus.size() && t.pi_chunk_index.size() == t.pi_chunk_locus.size() &&
              t.locus_pichunk_offsets.size() == offsets.size() && t.locus_pichunk_offsets.back() == (int64_t)t.pi_chunk_locus.size();
    for (size_t c = 0; ok && c < t.pi_chunk_locus.size(); ++c) {
        const int32_t l = t.pi_chunk_locus[c];
        ok = (int64_t)c - t.locus_pichunk_offsets[l] == t.pi_chunk_index[c] &&
             (int64_t)t.pi_chunk_index[c] * kPiChunk < offsets[l + 1] - offsets[l];
    }
    printf("chunk_tables_ok %d\n", ok ? 1 : 0);
    printf("grid %lld\n", (long long)site_grid(s, (int64_t)t.site_chunk_locus.size()));
    printf("lds_bytes %zu\nmixed_lds_bytes %zu\n", site_lds_bytes(s.lds_depth), mixed_lds_bytes(shape.stack_depth));
    // what launch_site_rates takes from these decisions at every launch
    const SiteKernelArgs a = site_kernel_args(s, shape.nwords, shape.stack_depth, (int64_t)t.site_chunk_locus.size());
    printf("site_variant %d\nargs.variant %d\nargs.lds_bytes %zu\nargs.grid %lld\nargs.persistent %d\nargs.first_round %d\n",
           site_variant(shape.nwords), a.variant, a.lds_bytes, (long long)a.grid, a.persistent, a.first_round);
    printf("args.first_fraction %.17g\nargs.tail_order %d\nargs.share_work %d\nargs.main_shares %d\nargs.spill %d\nargs.second_list %d\n",
           a.first_fraction, a.tail_order, a.share_work, a.main_shares, a.spill ? 1 : 0, a.second_list ? 1 : 0);
    const std::pair<const char*, size_t> regions[] = {
        {"work_cols", w.work_cols}, {"work_cols2", w.work_cols2}, {"work_count", w.work_count}, {"work_prefix", w.work_prefix},
        {"slice_prefix", w.slice_prefix}, {"work_class", w.work_class}, {"work_wprefix", w.work_wprefix}, {"part_prefix", w.part_prefix},
        {"part_start", w.part_start}, {"chunk_cnt", w.chunk_cnt}, {"partial", w.partial}, {"packed", w.packed}, {"hash", w.hash},
        {"dup_of", w.dup_of}, {"tab_key", w.tab_key}, {"tab_val", w.tab_val}, {"dedup_on", w.dedup_on}, {"spill", w.spill},
        {"total", w.total}};
    for (const auto& r : regions) printf("ws.%s %zu\n", r.first, r.second);
    return 0;
}
