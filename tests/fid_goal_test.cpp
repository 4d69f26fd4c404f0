// Prints the fidelity constants g_r, g_i and the normaliser n that qc_fidelity_goal (csrc/qc_side.h) makes of a goal: the one
// definition behind qc_fidelity_create_desc, qc_fidelity_create_kind and qc_sweep_create, on the CPU.
//   fid_goal_test <kind> <N> <goal file: doubles, one per line> [subspace level ...]
// Output: n, then one line per entry "g_r g_i" with 17 significant digits.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "qc_side.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int kind = atoi(argv[1]), N = atoi(argv[2]);
    std::vector<double> goal;
    FILE* f = fopen(argv[3], "r");
    if (!f) return 2;
    for (double v; fscanf(f, "%lf", &v) == 1;) goal.push_back(v);
    fclose(f);
    std::vector<int32_t> sub;
    for (int k = 4; k < argc; ++k) sub.push_back(atoi(argv[k]));
    const size_t len = kind == QC_FID_UNITARY ? 2 * (size_t)N * N : 2 * (size_t)N;
    std::vector<double> gr(len, -7.0), gi(len, -7.0);      // (the function fills every entry)
    const int n = qc_fidelity_goal(kind, N, goal.data(), sub.empty() ? nullptr : sub.data(), (int)sub.size(), gr.data(), gi.data());
    printf("%d\n", n);
    for (size_t i = 0; i < len; ++i) printf("%.17g %.17g\n", gr[i], gi[i]);
    return 0;
}
