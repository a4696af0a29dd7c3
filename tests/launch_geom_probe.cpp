// Prints the step forms and every launch geometry of csrc/sm_launch.h for a table of inputs (tests/test_launch_geom_cpu.py reads it).
// Host code only.  Usage: launch_geom_probe vn_fold_cap stream_tpr chain_cols graph_cap lin6_chunk  -- the kernel headers' constants.
// One row of integers per point, the columns named by the first line; a point = (variant, num_cu, KP, H, mode, N), where a variant
// is the default options with one option changed.  fold and graph_fused depend on max_mol_atoms too: one bit per value of kMaxMol.
#include "../shapemol_amd/csrc/sm_launch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

const int kMaxMol[] = {0, 1, 2, 33, 97, 128, 129, 121, 122};      // (121 | 122: the fold's boundary for the 16 atoms of eight one-job waves at KP = 8)

struct Variant { const char *name; int mode; int lg::Options::*field; int value; bool fits; };      // mode: -1 both, 0 exact, 1 f16x2
const Variant kVariants[] = {
    {"default", -1, nullptr, 0, true},
    {"edge_tiles", 1, &lg::Options::edge_tiles, 0, true},
    {"edge_waves", 1, &lg::Options::edge_threads, 6 * 64, true},
    {"lin_fuse", 1, &lg::Options::lin_fuse, 1, true},
    {"chain16_does_not_fit", 1, nullptr, 0, false},
    {"stream_chunk", 0, &lg::Options::stream_chunk_opt, 3, true},
    {"stream_whole_rounds", 0, &lg::Options::stream_whole_rounds, 1, true},
    {"x2h_out_fuse_0", 0, &lg::Options::x2h_out_fuse, 0, true},
    {"x2h_out_fuse_2", 0, &lg::Options::x2h_out_fuse, 2, true},
    {"node_levels", 0, &lg::Options::node_levels, 0, true},
    {"after_waves", 0, &lg::Options::after_waves, 8, true},
    {"after_lin_wgs", 0, &lg::Options::after_lin_wgs, 100, true},
};

// every N up to the last form switch of this CU count (the f16 kernels loop beyond 12 jobs per CU of two atoms; at 4 CUs the
// streaming workgroups outgrow the fused tail at 96 atoms and the fold's table at 256), plus 40
int n_max(int num_cu) { return (num_cu == 4 ? 4 * 256 : num_cu * 24) + 41; }

const char *kColumns =
    "variant num_cu KP H mode N fused_prologue f16 stream phases half_tiles lin_fused levels out_fused xc_fused fold_bits graph_fused_bits "
    "s_jobs s_chunk s_grid s_apw e_form e_jobs e_waves e_grid e_chunk e_slice e_apw e_last_grid x_form x_jobs x_waves x_grid x_apw "
    "p_form p_jobs p_waves p_grid p_chunk q_jobs q_waves q_grid l_n_ct l_ogroups l_tpg l_agroups n_n_ct n_pairs n_bw n_fjobs n_ljobs n_tpg n_lin_chunk";

}  // namespace

int main(int argc, char **argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: launch_geom_probe vn_fold_cap stream_tpr chain_cols graph_cap lin6_chunk\n"); return 2; }
    lg::KernelConsts kc{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), true};
    std::printf("%s\n", kColumns);
    for (const Variant &v : kVariants) std::printf("# %s\n", v.name);
    std::vector<long> row;
    int vi = 0;
    for (const Variant &v : kVariants) {
        for (int num_cu : {4, 64, 256, 304}) {
            if (vi > 0 && num_cu > 64) continue;      // the variants: the two small CU counts reach every switch
            for (int KP : {8, 16, 32}) for (int H : {32, 128}) for (int mode = 0; mode < 2; ++mode) {
                if (v.mode >= 0 && v.mode != mode) continue;
                for (int N = 1; N <= n_max(num_cu); ++N) {
                    lg::In in{lg::Options{}, kc, KP, num_cu, H, N};
                    in.k.chain16_fits = v.fits;
                    in.o.edge_bf16 = mode ? 3 : 2; in.o.node_f16 = mode;
                    if (v.field) in.o.*v.field = v.value;
                    long fold = 0, gf = 0;
                    for (size_t m = 0; m < sizeof(kMaxMol) / sizeof(int); ++m) {
                        in.o.max_mol_atoms = kMaxMol[m];
                        const lg::StepForms f = lg::step_forms(in, true, false);
                        fold |= (long)f.fold << m; gf |= (long)f.graph_fused << m;
                    }
                    const lg::StepForms f = lg::step_forms(in, true, false);      // (the other forms do not depend on max_mol_atoms)
                    const lg::StreamGeom s = lg::stream_geom(in);
                    const lg::EdgeGeom e = lg::edge16_geom(in), x = lg::x2h_chain_geom(in), p = lg::edge_phase_geom(in), q = lg::edge_fp32_geom(in);
                    const int last = (e.jobs - 1) / e.slice * e.slice;
                    const lg::LinGeom l = lg::linear_geom(in, 8 * (H / 16));
                    const lg::NodeLevelsGeom n = lg::node_levels_geom(in, 2, 8 * (H / 16));
                    row = {vi, num_cu, KP, H, mode, N, f.fused_prologue, f.f16, f.stream, f.phases, f.half_tiles, f.lin_fused, f.levels, f.out_fused, f.xc_fused, fold, gf,
                           s.jobs, s.chunk, s.grid, s.atoms_per_wg, (long)e.form, e.jobs, e.waves, e.grid, e.chunk, e.slice, e.atoms_per_wg, lg::slice_grid(e, last),
                           (long)x.form, x.jobs, x.waves, x.grid, x.atoms_per_wg, (long)p.form, p.jobs, p.waves, p.grid, p.chunk, q.jobs, q.waves, q.grid,
                           l.n_ct, l.ogroups, l.tpg, l.agroups, n.n_ct, n.n_pairs, n.bw, n.n_fjobs, n.n_ljobs, n.tpg, n.lin_chunk};
                    for (size_t i = 0; i < row.size(); ++i) std::printf(i ? " %ld" : "%ld", row[i]);
                    std::printf("\n");
                }
            }
        }
        ++vi;
    }
    return 0;
}
