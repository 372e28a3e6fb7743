// Test helper (host only): how the replicate-band stages cut their work to a workspace (tapir_amd/csrc/band_blocks.hpp), walked
// the way the drivers walk it.  Reads one query per line from stdin; `at` is the workspace's address, `d` its size as bytes
// above the minimum (-1: the preferred size).  Prints per query
//   base <at> <bytes>                                  -> <aligned address> <usable>
//   bs <at> <d> <tile> <T> <n_i> <B> <L> <sizes...>    -> <min> <preferred> <usable after the ids> <blocks> {<l0> <l1> <range>}
//   rs <at> <d> <n_i> <L> <sizes...>                   -> <min> <preferred> <usable> <blocks> {<l0> <l1>}
//   pp <at> <d> <Wb> <K> <B> <L>                       -> <min> <preferred> <usable after the ids> <loci per block>
//   pb <ntaxa> <ncols> <nloci> <W> <Wb> <B> <plan ws>  -> the twelve fields of ParbootLayout
#include <cstdio>
#include <cstring>
#include <vector>
#include "band_blocks.hpp"

using namespace tphip;

static long long next() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) return 0;
    return v;
}

static std::vector<int64_t> read_offsets(long long L) {
    std::vector<int64_t> off(1, 0);
    for (long long l = 0; l < L; ++l) off.push_back(off.back() + next());
    return off;
}

static size_t usable_of(long long at, long long d, const BandBytes& W) {
    return band_base((uintptr_t)at, d < 0 ? W.preferred : W.min + (size_t)d).usable;
}

int main() {
    char what[8];
    while (scanf("%7s", what) == 1) {
        if (!strcmp(what, "base")) {
            const long long at = next(), bytes = next();
            const BandBase b = band_base((uintptr_t)at, (size_t)bytes);
            printf("%llu %zu\n", (unsigned long long)b.base, b.usable);
        } else if (!strcmp(what, "bs")) {
            const long long at = next(), d = next(), tile = next(), T = next(), n_i = next(), B = next(), L = next();
            const std::vector<int64_t> off = read_offsets(L);
            const int32_t Wb = (int32_t)(T + n_i);
            const BandBytes W = bootstrap_bytes(off.data(), L, (int32_t)n_i, Wb, B, tile);
            const size_t usable = usable_of(at, d, W) - band_ids_bytes(L);
            std::vector<long long> out;
            for (int64_t l0 = 0; l0 < L;) {
                const BsBlock k = bootstrap_next_block(off.data(), L, l0, (int32_t)n_i, Wb, B, tile, usable);
                out.insert(out.end(), {l0, k.l1, k.range});
                l0 = k.l1;
            }
            printf("%zu %zu %zu %zu", W.min, W.preferred, usable, out.size() / 3);
            for (long long v : out) printf(" %lld", v);
            printf("\n");
        } else if (!strcmp(what, "rs")) {
            const long long at = next(), d = next(), n_i = next(), L = next();
            const std::vector<int64_t> off = read_offsets(L);
            int64_t longest = 0;
            for (long long l = 0; l < L; ++l) longest = std::max(longest, off[l + 1] - off[l]);
            const BandBytes W = resample_bytes(longest, off[L], (int32_t)n_i);
            const size_t usable = usable_of(at, d, W);
            std::vector<long long> out;
            for (int64_t l0 = 0; l0 < L;) {
                const int64_t l1 = resample_next_block(off.data(), L, l0, (int32_t)n_i, usable);
                out.insert(out.end(), {l0, l1});
                l0 = l1;
            }
            printf("%zu %zu %zu %zu", W.min, W.preferred, usable, out.size() / 2);
            for (long long v : out) printf(" %lld", v);
            printf("\n");
        } else if (!strcmp(what, "pp")) {
            const long long at = next(), d = next(), Wb = next(), K = next(), B = next(), L = next();
            const BandBytes W = posterior_bytes(L, (size_t)K, (size_t)B, (size_t)Wb);
            const size_t usable = usable_of(at, d, W) - band_ids_bytes(L ? L : 1);
            printf("%zu %zu %zu %zu\n", W.min, W.preferred, usable, posterior_block_loci((size_t)L, (size_t)K, (size_t)B, (size_t)Wb, usable));
        } else if (!strcmp(what, "pb")) {
            const long long ntaxa = next(), ncols = next(), nloci = next(), W = next(), Wb = next(), B = next(), ws = next();
            const ParbootLayout P = parboot_layout((size_t)ntaxa, (size_t)ncols, (size_t)nloci, (size_t)W, (size_t)Wb, (size_t)B, (size_t)ws);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", P.states, P.rate, P.subst, P.lnl, P.flag, P.nres, P.tables, P.rows,
                   P.mean, P.m2, P.plan_ws, P.total);
        } else {
            return 2;
        }
    }
    return 0;
}
