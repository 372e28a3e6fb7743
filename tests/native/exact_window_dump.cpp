// Host build of tapir_amd/csrc/exact_quartet_window.hpp, the window rule the moment kernel of the exact quartet probabilities
// runs on the device.  Reads lines "v1 v2 ve cap tol" and prints "M bound" with 17 digits each.
#include <cstdio>

#include "exact_quartet_window.hpp"

int main() {
    double v1, v2, ve, tol;
    int cap;
    while (std::scanf("%lf %lf %lf %d %lf", &v1, &v2, &ve, &cap, &tol) == 5) {
        if (!tphip::exact_window_valid(cap)) {
            std::printf("invalid\n");
            continue;
        }
        double bound = -1.0;
        const int m = tphip::exact_window(v1, v2, ve, cap, tol, &bound);
        std::printf("%d %.17g\n", m, bound);
    }
    return 0;
}
