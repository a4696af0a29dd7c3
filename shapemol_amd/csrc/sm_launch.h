// Launch geometry and step forms of one score evaluation: plain host C++17, no HIP types, no kernel templates.
// Every launcher of shapemol_hip.hip takes its waves, grid and chunk from a struct computed here, and every decision that
// depends on such a number (fold, xc_fused, out_fused: step_forms) reads the same struct -- so the two cannot disagree.
// Constants that live in kernel headers enter as plain numbers (KernelConsts); tests/launch_geom_probe.cpp builds this header
// alone and prints everything below for a table of inputs (tests/test_launch_geom_cpu.py).
#pragma once
#include <algorithm>

namespace lg {

// The options of a context that select kernels and shape launches (shapemol_set_option)
struct Options {
    int stop_layer = -1, edge_threads = 0 /* 0 = chosen per launch */, lin_waves = 16, edge_bf16 = 2, lin_bf16 = 1, chain_bf16 = 1, vn_fuse = 2;
    int vn_fold = 1;            // coordinate update of layer l in the prologue of the x2h kernel of layer l + 1 (needs max_mol_atoms)
    int max_mol_atoms = 0;      // largest molecule of the batches to come (option; 0 = unknown: no fold)
    int stream_whole_rounds = 0;   // streaming edge kernels: 1 = tiles per workgroup rounded up to whole rounds.  0 (default): as many workgroups as
                                   // the tiles give; the last round of an odd chunk has one tile (B = 256: 252 workgroups of 11 tiles instead of
                                   // 231 of 12 -- x2h 26.7 -> 25.6 us, h2x 24.7 -> 23.9; B = 1024, 43 instead of 44: unchanged)
    int lin_fuse = 0;           // 1: per-node products of the next attentions inside node_chain16_kernel instead of a node_linear
    int ddpm_fold = 1;          // 1: the last layer's coordinate update inside the DDPM kernel (chains without guidance)
    int graph_fuse = 1;         // 1: kNN graph + edge weights in one launch (graph_kernel) when max_mol_atoms <= kGraphCap is known
    int x2h_chain = 1;          // 1: x2h attention and the node stage of a layer in one launch (x2h_chain16_kernel) when every wave has one job
                                // launch (measured: 28.5 us against 15.3 + 11.1 us, eight dependent weight blocks per wave)
    int node_levels = 1;        // 1: the exact-mode node stage as node_out6_kernel (h' only) + node_after6_kernel (follow-up MLPs and per-node products
                                // side by side); 0: node_chain6_kernel + node_linear6_kernel
    int x2h_out_fuse = 1;       // 1: h' inside the x2h streaming kernel's tail (stream_node_out_epilogue) instead of a node_out6_kernel launch, while a
                                // workgroup owns at most 3 * CHAIN_COLS * 16 (96) atoms; 2: whatever it owns (measurements); 0: node_out6_kernel
    int stream_chunk_opt = 0;   // option "stream_chunk": tiles per workgroup of the streaming kernels (tests); 0 = automatic
    int after_order = 2;        // node_after6_kernel's grid: 0 follow-up jobs first, 1 interleaved with the linear jobs, 2 linear jobs first
    int after_waves = 16;       // ... waves of its linear jobs (the workgroup has max(H / 16, after_waves) waves)
    int after_lin_wgs = 0;      // ... workgroups aimed at for its linear jobs (0 = automatic)
    int node_f16 = 0;           // 1: node kernels on two-piece f16 operands (sm_node16.h) instead of exactly split bf16 (sm_node.h) [default 0]
    int feat_f16 = 0;           // 1: "f16 features" -- matrix products on the leading f16 piece only (one product per term instead of
                                // three; accumulation, LayerNorm, softmax, coordinates fp32).  Reduced precision, NOT a parity mode
    int edge_tiles = -1;        // f16 edge kernels when the waves have several jobs: 0 = sliced launches of the one-job kernel,
                                // 1 = one looping launch (eight waves per workgroup, next job's rows prefetched), -1 = automatic (= 1) [default]
    int prologue_tab = 1;       // 1: the per-step node prologue gathers from the tables; 0: the per-atom MLP kernel
};

// What the kernel headers fix: kVnFoldCap, kStreamTPR, CHAIN_COLS, kGraphCap, kLin6Chunk, and whether the node stage's LDS fits
// inside the two edge images of x2h_chain16_kernel (Chain16Lds<H>::BYTES <= 2 * EdgeImage16<H, H / 16>::TOTAL * 4)
struct KernelConsts { int vn_fold_cap, stream_tpr, chain_cols, graph_cap, lin6_chunk; bool chain16_fits; };

struct In { Options o; KernelConsts k; int KP, num_cu, H, n_atoms; };

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// A job = one 16-slot tile: 16 / KP centre atoms (k <= 16), or half an atom (k > 16: two tiles per atom, merged afterwards)
struct Jobs { int apj, jobs; bool half; };
inline Jobs tile_jobs(int KP, int n_atoms) {
    const int apj = KP >= 16 ? 1 : 16 / KP;
    return {apj, KP > 16 ? 2 * n_atoms : cdiv(n_atoms, apj), KP > 16};
}

// An edge launch.  One: every wave has at most one job (`chunk` = waves jobs per workgroup); Loop: a workgroup owns `chunk`
// consecutive jobs; Sliced: several One launches over `slice` = grid x waves jobs each; Strided: the workgroups stride over the
// jobs, `chunk` at a time.  atoms_per_wg: the consecutive whole atoms one workgroup owns (0: half-atom tiles, Strided)
enum class Form { One, Loop, Sliced, Strided };
struct EdgeGeom { Form form; int apj, jobs, waves, grid, chunk, slice, atoms_per_wg; };

// Waves per workgroup of the single-tile edge kernels: one job per wave while the jobs fit (the launch then lasts
// one job latency), on as many CUs as possible: ceil(jobs / CUs) waves, at least 4 and at most 12 (the 168-VGPR budget).
inline int edge_waves(const In &in, int jobs) {
    return in.o.edge_threads > 0 ? in.o.edge_threads / 64 : std::max(4, std::min(12, cdiv(jobs, in.num_cu)));
}
inline EdgeGeom one_job_geom(const In &in, int waves) {      // as many workgroups of `waves` one-job waves as the jobs need, one per CU at most
    const Jobs j = tile_jobs(in.KP, in.n_atoms);
    const int grid = std::max(1, std::min(in.num_cu, cdiv(j.jobs, waves)));
    return {j.jobs <= grid * waves ? Form::One : Form::Strided, j.apj, j.jobs, waves, grid, waves, grid * waves, j.half ? 0 : waves * j.apj};
}

// fp32-MFMA edge kernel (edge_bf16 = 0): one job per workgroup at a time
inline EdgeGeom edge_fp32_geom(const In &in) {
    const Jobs j = tile_jobs(in.KP, in.n_atoms);
    const int grid = std::max(1, std::min(in.num_cu, j.jobs));
    return {Form::Strided, j.apj, j.jobs, in.o.edge_threads > 0 ? in.o.edge_threads / 64 : 12, grid, 1, grid, 0};
}

// phase kernels (edge_bf16 = 1): the straight-line instantiation while every wave has one job, else strided
inline EdgeGeom edge_phase_geom(const In &in) {
    EdgeGeom g = one_job_geom(in, edge_waves(in, tile_jobs(in.KP, in.n_atoms).jobs));
    if (g.form == Form::Strided) g.atoms_per_wg = 0;
    return g;
}

// two-piece f16 edge kernels (edge_bf16 = 3): one launch of the straight-line instantiation; beyond that (edge_tiles) one looping
// launch -- eight waves per workgroup (two per SIMD, 256 VGPRs: a job's state plus the next job's gathered rows without spilling)
// -- or slices of equal size: the jobs spread evenly over the fewest launches that can hold them (a last slice that is nearly
// empty costs a full launch floor; no spills, full overlap inside a launch; the image fill is paid per slice)
inline EdgeGeom edge16_geom(const In &in) {
    EdgeGeom g = one_job_geom(in, edge_waves(in, tile_jobs(in.KP, in.n_atoms).jobs));
    if (g.form == Form::One) return g;
    const int cu = in.num_cu, et = in.o.edge_threads;
    if (in.o.edge_tiles != 0) {      // (-1 = automatic: looping)
        g.form = Form::Loop;
        g.waves = et > 0 ? std::min(8, et / 64) : 8;
        g.chunk = cdiv(g.jobs, std::max(1, std::min(cu, cdiv(g.jobs, g.waves))));
        g.grid = cdiv(g.jobs, g.chunk);
        g.slice = g.jobs;
    } else {
        g.form = Form::Sliced;
        if (et == 0) {      // (an explicit edge_waves option keeps its wave count)
            const int target = cdiv(g.jobs, cdiv(g.jobs, cu * 12));
            g.waves = std::max(4, std::min(12, cdiv(target, cu)));
            g.grid = std::max(1, std::min(cu, cdiv(target, g.waves)));
        }
        g.chunk = g.waves;
        g.slice = g.grid * g.waves;
    }
    g.atoms_per_wg = in.KP > 16 ? 0 : g.chunk * g.apj;
    return g;
}
inline int slice_grid(const EdgeGeom &g, int base) {      // workgroups of the slice that starts at job `base` (One: the only one)
    return std::max(1, std::min(g.grid, cdiv(std::min(g.jobs, base + g.slice) - base, g.waves)));
}

// x2h attention + node stage in one launch (x2h_chain16_kernel): a workgroup has at least H / 16 waves (the node stage's output
// blocks).  One launch only (form One): in slices the fused kernel loses to the separate ones, whose node stage then has enough
// atoms per launch to run at its throughput (B = 1024: 523 against 538 molecules/s)
inline EdgeGeom x2h_chain_geom(const In &in) {
    EdgeGeom g = one_job_geom(in, std::max(in.H / 16, edge_waves(in, tile_jobs(in.KP, in.n_atoms).jobs)));
    if (g.form != Form::One) g.form = Form::Sliced;
    return g;
}

// streaming edge kernels (sm_edge_stream.h; edge_bf16 = 2): `chunk` consecutive tiles per workgroup -- every CU one workgroup;
// half-atom tiles (k > 16) in whole rounds of stream_tpr
struct StreamGeom { int jobs, chunk, grid, atoms_per_wg; };
inline StreamGeom stream_geom(const In &in) {
    const Jobs j = tile_jobs(in.KP, in.n_atoms);
    const int tpr = in.k.stream_tpr, opt = in.o.stream_chunk_opt, per_cu = cdiv(j.jobs, in.num_cu);
    int chunk;
    if (opt > 0) chunk = in.KP <= 16 ? opt : cdiv(opt, tpr) * tpr;
    else if (!in.o.stream_whole_rounds && in.KP <= 16) chunk = std::max(1, per_cu);
    else chunk = std::max(tpr, cdiv(per_cu, tpr) * tpr);
    return {j.jobs, chunk, cdiv(j.jobs, chunk), j.half ? 0 : chunk * j.apj};
}

// node_linear kernels: `ogroups` groups of lin_waves output tiles x `agroups` groups of `tpg` 16-atom column tiles, about one
// workgroup per CU
struct LinGeom { int n_ct, waves, ogroups, tpg, agroups; };
inline LinGeom linear_geom(const In &in, int n_out_tiles) {
    const int waves = in.o.lin_waves, n_ct = cdiv(in.n_atoms, 16), ogroups = cdiv(n_out_tiles, waves);
    const int tpg = std::max(1, cdiv(n_ct, std::max(1, in.num_cu / ogroups)));
    return {n_ct, waves, ogroups, tpg, cdiv(n_ct, tpg)};
}

// The exact-mode node stage in two levels: node_out6_kernel over `n_pairs` groups of CHAIN_COLS column tiles, then
// node_after6_kernel: n_follow follow-up jobs per pair beside linear jobs of `tpg` column tiles (staged `lin_chunk` at a time) in
// workgroups of `bw` waves.  The linear jobs fill the workgroup slots that the follow-up jobs leave, at least half of all
constexpr int kAfterChunk = 6;      // linear staging chunk of 8-wave workgroups: 6 * 3 * H * 32 = 72 KB at H = 128, two workgroups per CU
struct NodeLevelsGeom { int n_ct, n_pairs, lw, bw, n_fjobs, n_ljobs, tpg, lin_chunk; };
inline NodeLevelsGeom node_levels_geom(const In &in, int n_follow, int lin_tiles) {
    NodeLevelsGeom g{};
    g.n_ct = cdiv(in.n_atoms, 16); g.n_pairs = cdiv(g.n_ct, in.k.chain_cols);
    g.lw = in.o.after_waves; g.bw = std::max(g.lw, in.H / 16);
    const int per_cu = g.bw <= 8 ? 2 : 1;                   // workgroups that share a CU (128 VGPRs per lane; LDS: kAfterChunk)
    const int slots = in.num_cu * per_cu;
    g.n_fjobs = n_follow * g.n_pairs;
    g.tpg = 1;
    if (lin_tiles > 0) {
        const int ogroups = cdiv(lin_tiles, g.lw);
        const int lin_wgs = in.o.after_lin_wgs > 0 ? in.o.after_lin_wgs : std::max(slots - g.n_fjobs, slots / 2);
        g.tpg = std::max(1, cdiv(g.n_ct, std::max(1, lin_wgs / ogroups)));
        g.n_ljobs = ogroups * cdiv(g.n_ct, g.tpg);
    }
    g.lin_chunk = std::min(g.tpg, per_cu == 2 ? kAfterChunk : in.k.lin6_chunk);
    return g;
}

// The decisions of one score evaluation that do not depend on the layer.  sampling: a reverse step of a chain (the max_mol_atoms
// hint is set for the batch of a chain; a score evaluation on other data must not trust a stale one); pins: pinned neighbour lists
struct StepForms {
    bool fused_prologue;      // embedding + first queries + first per-node products in one launch
    bool graph_fused;         // kNN graph + edge weights in one launch (graph_kernel)
    bool fold;                // coordinate update of layer l inside the x2h kernel of layer l + 1
    bool f16, stream, phases; // two-piece f16 kernels (sm_edge16.h); streaming kernels (sm_edge_stream.h), the default; single-tile kernels
    bool half_tiles;          // k > 16: two 16-slot tiles per atom + combine
    bool lin_fused;           // per-node products inside node_chain16_kernel
    bool levels;              // two-level exact-mode node stage
    bool out_fused;           // h' computed by the streaming x2h kernel's tail
    bool xc_fused;            // x2h attention + node stage in one launch
};
inline StepForms step_forms(const In &in, bool sampling, bool pins) {
    const Options &o = in.o;
    const int KP = in.KP, m = o.max_mol_atoms;
    StepForms f{};
    f.fused_prologue = o.chain_bf16 && o.lin_bf16;
    f.graph_fused = sampling && o.graph_fuse && m > 0 && m <= in.k.graph_cap && KP <= 32 && !pins;
    f.f16 = o.edge_bf16 == 3; f.stream = o.edge_bf16 == 2; f.phases = o.edge_bf16 && KP <= 16;
    f.half_tiles = (f.f16 || f.stream) && KP > 16;
    f.lin_fused = o.chain_bf16 && o.lin_bf16 && o.node_f16 && o.lin_fuse;
    f.levels = o.node_levels && o.chain_bf16 && o.lin_bf16 && !o.node_f16 && !f.lin_fused;
    const StreamGeom sg = stream_geom(in);
    const EdgeGeom e16 = edge16_geom(in), xc = x2h_chain_geom(in);
    // one launch in which every wave has one job, on f16 node kernels; a workgroup's atoms fit the node stage's CHAIN_COLS column tiles
    f.xc_fused = f.f16 && o.x2h_chain && KP <= 16 && o.chain_bf16 && o.node_f16 && !o.lin_fuse && o.edge_threads == 0 &&
                 xc.form == Form::One && xc.waves <= 12 && xc.atoms_per_wg <= in.k.chain_cols * 16 && in.k.chain16_fits;
    // only where the two-level node form follows a streaming x2h kernel of whole-atom tiles.  The tail walks a workgroup's atoms 32
    // at a time and streams the output MLP's weights again for every pass; it won at every size measured, up to the 88 atoms (three
    // passes) of B = 1024, so the boundary is three passes: beyond that nothing is measured
    f.out_fused = f.stream && o.x2h_out_fuse && f.levels && KP <= 16 && (o.x2h_out_fuse == 2 || sg.atoms_per_wg <= 3 * in.k.chain_cols * 16);
    // the fold needs the VN-linear + statistics epilogue in h2x and every workgroup's molecule span -- its own atoms and the rest of
    // the molecules at both ends -- inside the LDS table of the x2h kernel.  f16: whichever x2h launch runs, the plain one or the one
    // fused with the node stage, so that the fold depends on the sizes alone (wave-count sweeps keep the plain path)
    const int own = f.stream ? sg.atoms_per_wg : std::max(e16.atoms_per_wg, xc.atoms_per_wg);
    f.fold = sampling && o.vn_fold && (f.f16 || f.stream) && KP <= 16 && o.vn_fuse == 2 && m > 0 && (f.stream || o.edge_threads == 0) &&
             own + 2 * (m - 1) <= in.k.vn_fold_cap;
    return f;
}

}  // namespace lg
