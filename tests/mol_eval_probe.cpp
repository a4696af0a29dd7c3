// Host program of tests/test_mol_eval_cpu.py: the host plan of the geometry scores and of the bond graphs (csrc/sm_mol_rule.h
// through csrc/sm_mol_eval.h and csrc/sm_mol_graph.h) without a GPU.
//   mol_eval_probe [graph] F n_0 n_1 ...      F frames of molecules with n_b atoms, the default histograms, a 2-element rule, 3 classes;
//                                             with `graph` the bond graph's plan: its limit on atoms, bond-length edges as well
// Prints "error <message>" and returns 1 when the plan refuses the call; else "mol b off n form" per molecule and one line
// "form <name> jobs gx iters" per launch form, then "jobs <name> b ..." with the molecules in job order.
#define SM_MOL_EVAL_HOST_ONLY
#include "../shapemol_amd/csrc/sm_mol_eval.h"
#include "../shapemol_amd/csrc/sm_mol_graph.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
    const bool graph = argc > 1 && !std::strcmp(argv[1], "graph");
    if (graph) { --argc; ++argv; }
    if (argc < 3) return 2;
    const int64_t F = std::atoll(argv[1]), B = argc - 2;
    std::vector<int64_t> off(B + 1, 0);
    for (int64_t b = 0; b < B; ++b) off[b + 1] = off[b] + std::atoll(argv[2 + b]);
    std::vector<double> cc(100), al(100), bl(161);
    for (int i = 0; i < 100; ++i) { cc[i] = 2.0 * i / 99; al[i] = 12.0 * i / 99; }
    for (int i = 0; i < 161; ++i) bl[i] = 0.8 + 0.01 * i;
    const int32_t slot[3] = {0, 1, 1};
    MolPlan pl;
    const std::string e = graph ? mgraph_plan(F, B, off.data(), 2, 3, slot, cc.data(), 100, 2.0, al.data(), 100, 12.0, bl.data(), 161, &pl)
                                : meval_plan(F, B, off.data(), 2, 3, slot, cc.data(), 100, 2.0, al.data(), 100, 12.0, &pl);
    if (!e.empty()) { std::printf("error %s\n", e.c_str()); return 1; }
    for (int64_t b = 0; b < B; ++b) std::printf("mol %lld %d %d %d\n", (long long)b, pl.mol[b].off, pl.mol[b].n, pl.form[b]);
    const MolForm *forms[2] = {&pl.wave, &pl.block};
    const char *names[2] = {"wave", "block"};
    for (int k = 0; k < 2; ++k) {
        std::printf("form %s %zu %d %d\n", names[k], forms[k]->jobs.size(), forms[k]->gx, forms[k]->iters);
        std::printf("jobs %s", names[k]);
        for (int b : forms[k]->jobs) std::printf(" %d", b);
        std::printf("\n");
    }
    return 0;
}
