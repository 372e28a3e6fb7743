// Test helper (host only): the later shares' cut of the reserved tails (tapir_amd/csrc/tail_shares.hpp) and what the launch
// decision makes of it (site_launch_plan.hpp), from records on stdin, one per line:
//   ranges <big> <mid> <small> <frac_big_q> <frac_mid_q> <ttotal> <kmax>
//       -> "ranges <count> <bound> <g0> <g1> ... " : tail_share_count(ttotal), tail_share_bound(ttotal) and the ranges of k = 0 .. kmax - 1
//   bound <big> <mid> <small> <frac_big_q> <frac_mid_q> <ttotal_max>
//       -> "bound <tail_share_bound>"
//   decide <ntaxa> <nwords> <stack_depth> <nloci> <columns each> <CUs> <workgroups per CU> [TPHIP_KNOB=text ...]
//       -> "decide <waves> <grid_mult> <share_work> <reserve_q> <big> <mid> <small> <frac_big_q> <frac_mid_q> <tail_share_bound> <grid> <spill bytes> <min_total>"
//          (every occupancy query answers <workgroups per CU>, the one for the spill variant two more)
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include "site_launch_plan.hpp"

using namespace tphip;

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        TailShares t;
        if (what == "ranges" || what == "bound") {
            long long ttotal = 0, kmax = 0;
            in >> t.fills_big >> t.fills_mid >> t.fills_small >> t.frac_big_q >> t.frac_mid_q >> ttotal;
            if (what == "bound") {
                if (!in) { fprintf(stderr, "bad line: %s", line); return 2; }
                printf("bound %lld\n", (long long)tail_share_bound(ttotal, t));
                continue;
            }
            in >> kmax;
            if (!in) { fprintf(stderr, "bad line: %s", line); return 2; }
            printf("ranges %lld %lld", (long long)tail_share_count(ttotal, t), (long long)tail_share_bound(ttotal, t));
            for (long long k = 0; k < kmax; ++k) {
                int64_t g0 = -1, g1 = -1;
                tail_share_range(k, ttotal, t, &g0, &g1);
                printf(" %lld %lld", (long long)g0, (long long)g1);
            }
            printf("\n");
        } else if (what == "decide") {
            SiteShape shape;
            long long nloci = 0, cols = 0;
            int cus = 0, per_cu = 0;
            in >> shape.ntaxa >> shape.nwords >> shape.stack_depth >> nloci >> cols >> cus >> per_cu;
            if (!in || cus < 1 || nloci < 1) { fprintf(stderr, "bad line: %s", line); return 2; }
            shape.nloci = nloci; shape.ncols = nloci * cols; shape.max_locus_cols = cols; shape.T = 50; shape.n_i = 2;
            PlanKnobs knobs;
            std::string kv;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                if (eq == std::string::npos || !set_plan_knob(&knobs, kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str())) {
                    fprintf(stderr, "no knob %s\n", kv.c_str());
                    return 2;
                }
            }
            const SiteLaunch s = decide_site_launch(shape, cus, knobs, [per_cu](int variant, size_t) { return variant == kStreamWordsSpill ? per_cu + 2 : per_cu; });
            const WorkspaceLayout w = layout_workspace(shape, s, 0);
            const size_t spill_bytes = s.lds_depth < shape.stack_depth ? w.total - 256 - w.spill : 0;
            printf("decide %d %d %d %d %d %d %d %d %d %lld %lld %zu %d\n", s.waves, s.grid_mult, s.share_work, s.reserve_q, s.tail_shares.fills_big,
                   s.tail_shares.fills_mid, s.tail_shares.fills_small, s.tail_shares.frac_big_q, s.tail_shares.frac_mid_q,
                   (long long)s.tail_share_bound, (long long)site_grid(s, 0), spill_bytes, s.tail_shares.min_total);
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
