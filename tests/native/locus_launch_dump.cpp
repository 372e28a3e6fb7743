// Test helper (host only): the stage-1 launch decisions of plan creation and the per-call arithmetic
// (tapir_amd/csrc/locus_launch_plan.hpp) for a shape, knobs and the kernels' answers read from stdin, one record per line:
//   shape <ntaxa> <nnodes> <nwords> <stack_depth> <ntape> <max_locus_cols> <value_nops> <grad2_built> <grad2_rdepth> <grad2_ntape>
//   cus <CU count>
//   knob <TPHIP_...> <text>                (the text an environment variable would hold)
//   allow <kernel> <lds_bytes> <0|1>       (kernel: lik, value, grad, grad2)
//   occ <kernel> <lds_bytes> <resident workgroups per CU>
//   nsplit <ncand> <max_locus_cols> <block>
//   layout <items> <nnodes> <want_dlogt 0|1> <want_d2logt 0|1>
// Prints the LocusLaunch fields as "name value" lines, the queries made of the two callables in order on one line, and one line
// per nsplit / layout record.  A query that the tables do not hold answers as a failed one does (not allowed / 0).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "locus_launch_plan.hpp"

using namespace tphip;

static const char* const kKernelNames[] = {"lik", "value", "grad", "grad2"};

static int kernel_of(const char* name) {
    for (int k = 0; k < 4; ++k) if (strcmp(name, kKernelNames[k]) == 0) return k;
    return -1;
}

int main() {
    LocusShape shape;
    PlanKnobs knobs;
    int cus = 0;
    std::map<std::pair<int, size_t>, int> allow, occ;
    std::vector<std::string> answers;
    char line[512], name[128], text[256];
    while (fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0, c = 0;
        int built = 0, x = 0, y = 0;
        if (sscanf(line, "shape %d %d %d %d %d %lld %d %d %d %d", &shape.ntaxa, &shape.nnodes, &shape.nwords, &shape.stack_depth, &shape.ntape,
                   &a, &shape.value_nops, &built, &shape.grad2_rdepth, &shape.grad2_ntape) == 10) {
            shape.max_locus_cols = a;
            shape.grad2_built = built != 0;
            continue;
        }
        if (sscanf(line, "cus %d", &cus) == 1) continue;
        if (sscanf(line, "allow %127s %lld %d", name, &a, &x) == 3 || sscanf(line, "occ %127s %lld %d", name, &a, &x) == 3) {
            const int k = kernel_of(name);
            if (k < 0) { fprintf(stderr, "no kernel %s\n", name); return 2; }
            (line[0] == 'a' ? allow : occ)[{k, (size_t)a}] = x;
            continue;
        }
        if (sscanf(line, "nsplit %lld %lld %lld", &a, &b, &c) == 3) {
            if (cus < 1) { fprintf(stderr, "nsplit needs cus before it\n"); return 2; }
            answers.push_back("nsplit " + std::to_string(a) + " " + std::to_string(b) + " " + std::to_string(c) + " -> " +
                              std::to_string(lik_nsplit(cus, b, a, (int)c)));
            continue;
        }
        if (sscanf(line, "layout %lld %lld %d %d", &a, &b, &x, &y) == 4) {
            const GradOutLayout g((size_t)a, (size_t)b, x != 0, y != 0);
            char buf[256];
            snprintf(buf, sizeof buf, "layout %lld %lld %d %d -> %zu %zu %zu %zu %zu total %zu", a, b, x, y, g.lnl, g.sum_dlogt, g.dexch, g.dlogt,
                     g.d2logt, g.total);
            answers.push_back(buf);
            continue;
        }
        text[0] = 0;
        if (sscanf(line, "knob %127s %255s", name, text) >= 1) {
            if (!set_plan_knob(&knobs, name, text)) { fprintf(stderr, "no knob %s\n", name); return 2; }
            continue;
        }
        if (line[0] != '\n') { fprintf(stderr, "bad line: %s", line); return 2; }
    }
    if (cus < 1 || shape.nnodes < 1) { fprintf(stderr, "need cus and shape\n"); return 2; }

    std::string queries;
    const LocusLaunch s = decide_locus_launch(
        shape, cus, knobs,
        [&](LocusKernel k, int cols, int depth, size_t lds) {
            queries += std::string(queries.empty() ? "" : "; ") + "allow " + kKernelNames[k];
            if (k == LOCUS_VALUE) queries += " " + std::to_string(cols);
            if (k == LOCUS_VALUE || k == LOCUS_GRAD2) queries += " " + std::to_string(depth);
            queries += " " + std::to_string(lds);
            const auto it = allow.find({(int)k, lds});
            return it != allow.end() && it->second != 0;
        },
        [&](LocusKernel k, int depth, size_t lds) {
            queries += std::string(queries.empty() ? "" : "; ") + "occ " + kKernelNames[k];
            if (k == LOCUS_GRAD2) queries += " " + std::to_string(depth);
            queries += " " + std::to_string(lds);
            const auto it = occ.find({(int)k, lds});
            return it == occ.end() ? 0 : it->second;
        });
    printf("lik_lds %zu\nlik_ok %d\nvalue_cols %d\nvalue_lds %zu\n", s.lik_lds, s.lik_ok ? 1 : 0, s.value_cols, s.value_lds);
    printf("grad_lds %zu\ngrad_stage %d\ngrad_slots %d\ngrad_blocks_per_cu %d\ngrad_ok %d\n", s.grad_lds, s.grad_stage, s.grad_slots,
           s.grad_blocks_per_cu, s.grad_ok ? 1 : 0);
    printf("grad2_ok %d\ngrad2_lds %zu\ngrad2_blocks_per_cu %d\n", s.grad2_ok ? 1 : 0, s.grad2_lds, s.grad2_blocks_per_cu);
    printf("queries %s\n", queries.c_str());
    // the per-call sizes for this shape: a million candidates (no column split), one tape per CU
    printf("value_chunk %lld\ngrad2_chunk %lld\n", (long long)value_chunk(shape.nnodes, 1000000, 1), (long long)grad2_chunk(shape.nnodes, 1000000));
    printf("grad_tape_bytes %zu\ngrad2_tape_bytes %zu\n", grad_tape_bytes(cus, shape.ntape, shape.stack_depth), grad2_tape_bytes(cus, shape.grad2_ntape));
    for (const std::string& a : answers) printf("%s\n", a.c_str());
    return 0;
}
