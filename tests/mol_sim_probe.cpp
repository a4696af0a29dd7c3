// Host program of tests/test_mol_sim_cpu.py: the host plan of the molecule similarity (csrc/sm_mol_sim.h) without a GPU.
//   mol_sim_probe MODE NA n_0 .. n_{NA-1} NB m_0 .. m_{NB-1} P a_0 b_0 a_1 b_1 ... [bad]
// MODE 0 shape, 1 esp (3 terms).  Set a has NA molecules of n_k atoms, set b NB of m_k; P pairs follow.  `bad` (optional):
// "alpha" a zero width, "nan" a NaN parameter, "term" a non-finite term, "terms" 17 terms.
// Prints "error <message>" and returns 1 when the plan refuses the call; else "pair p a b form al_off" per pair, "list <form>
// p ..." per launch form, then the jobs of an overlay with include_given: "job <stage> <form> xs xo xp xn ys yo yp yn out".
#define SM_MOL_SIM_HOST_ONLY
#include "../shapemol_amd/csrc/sm_mol_sim.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

int main(int argc, char **argv) {
    int k = 1;
    auto next = [&]() -> long long { return k < argc ? std::atoll(argv[k++]) : -1; };
    const int mode = (int)next();
    std::vector<int64_t> off[2];
    for (int s = 0; s < 2; ++s) {
        const long long n = next();
        off[s].assign(1, 0);
        for (long long m = 0; m < n; ++m) off[s].push_back(off[s].back() + next());
    }
    const long long P = next();
    std::vector<int64_t> pairs;
    for (long long p = 0; p < 2 * P; ++p) pairs.push_back(next());
    const char *bad = k < argc ? argv[k] : "";
    std::vector<double> u[2], v[2];
    for (int s = 0; s < 2; ++s) { u[s].assign((size_t)off[s].back(), 0.81); v[s].assign((size_t)off[s].back(), 0.8); }
    if (!std::strcmp(bad, "alpha") && !u[1].empty()) u[1].back() = 0.0;
    if (!std::strcmp(bad, "nan") && !v[0].empty()) (mode == MSIM_SHAPE ? v[0] : u[0])[0] = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> cA(17, 1.0), cB(17, 0.1);
    if (!std::strcmp(bad, "term")) cB[2] = std::numeric_limits<double>::infinity();
    const int K = mode == MSIM_ESP ? (!std::strcmp(bad, "terms") ? 17 : 3) : 0;
    const MsimSet a{(int64_t)off[0].size() - 1, off[0].data(), u[0].data(), mode == MSIM_SHAPE ? v[0].data() : nullptr};
    const MsimSet b{(int64_t)off[1].size() - 1, off[1].data(), u[1].data(), mode == MSIM_SHAPE ? v[1].data() : nullptr};
    MsimPlan pl;
    const std::string e = msim_plan(mode, a, b, P, pairs.data(), K, cA.data(), cB.data(), &pl);
    if (!e.empty()) { std::printf("error %s\n", e.c_str()); return 1; }
    for (size_t p = 0; p < pl.pairs.size(); ++p) std::printf("pair %zu %d %d %d %d\n", p, pl.pairs[p].a, pl.pairs[p].b, pl.form[p], pl.pairs[p].al_off);
    for (int f = 0; f < 2; ++f) {
        std::printf("list %d", f);
        for (int p : pl.list[f]) std::printf(" %d", p);
        std::printf("\n");
    }
    std::printf("aligned %lld\n", (long long)pl.n_aligned);
    const int Ma = (int)a.n_mols, Mb = (int)b.n_mols;
    std::vector<MsimJob> self[2], cross[2];
    msim_self_jobs(pl, self);
    msim_cross_jobs(pl, 2, Ma + Mb, cross);
    msim_cross_jobs(pl, 0, Ma + Mb + (int)P, cross);
    for (int stage = 0; stage < 2; ++stage)
        for (int f = 0; f < 2; ++f)
            for (const MsimJob &j : (stage ? cross : self)[f])
                std::printf("job %d %d %d %d %d %d %d %d %d %d %d\n", stage, f, j.xs, j.xo, j.xp, j.xn, j.ys, j.yo, j.yp, j.yn, j.out);
    return 0;
}
