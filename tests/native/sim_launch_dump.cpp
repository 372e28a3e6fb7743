// Test helper (host only): how the column simulation (tapir_amd/csrc/simulate_launch_shape.hpp) is launched for a tree with a
// given number of internal nodes.  Reads internal-node counts from stdin, one per line; prints per count
//   <nint> <ok 0/1> <words> <block> <dynamic LDS bytes> <1 if the launch must raise the kernel's LDS limit first>
#include <cstdio>
#include "simulate_launch_shape.hpp"

using namespace tphip;

int main() {
    long long n = 0;
    while (scanf("%lld", &n) == 1) {
        int32_t words = 0, block = 0;
        const bool ok = sim_launch_shape((int32_t)n, &words, &block);
        const size_t lds = sim_lds_bytes(words, block);
        printf("%lld %d %d %d %zu %d\n", n, ok ? 1 : 0, words, block, lds, lds > kSimLdsDefaultBytes ? 1 : 0);
    }
    return 0;
}
