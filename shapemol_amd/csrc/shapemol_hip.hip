// libshapemol_hip.so -- C ABI (include/shapemol_hip.h) over the gfx950 kernels.
// Host side: weight repacking into MFMA-friendly images, workspace, launch sequences for one
// score evaluation (ScorePosNet3D.forward) and for the reverse chain (sample_diffusion), hipGraph
// capture of one chain step, per-kernel event timing.
#include "../../include/shapemol_hip.h"
#include "sm_device.h"
#include "sm_edge.h"
#include "sm_edge_bf16.h"
#include "sm_edge16.h"
#include "sm_node.h"
#include "sm_node16.h"
#include "sm_edge_stream.h"
#include "sm_misc.h"
#include "sm_cfg.h"
#include "sm_guide_groups.h"      // (shape guidance stays behind the other kernel headers: DESIGN.md section 13, layout note)
#include "sm_mesh.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "sm_pack.h"
#include "sm_devmem.h"
#include "sm_host.h"
#include "sm_launch.h"

namespace {

#define HIPCHK SMCHK      // (sm_fail stores the message through shapemol_set_error_, below, where fail of sm_pack.h assigns g_err)
int hip_fail(const char *what, hipError_t e) { return fail(std::string(what) + ": " + hipGetErrorString(e)); }

constexpr int kEdgeThreadsDefault = 768;
#ifndef SM_GRAPH_UNROLL
#define SM_GRAPH_UNROLL 20
#endif
constexpr int kGraphUnroll = SM_GRAPH_UNROLL;   // reverse steps per graph launch

struct ProfRec { const char *name; hipEvent_t e0, e1; };

enum class Guide { None, Cloud, Mesh, Field, Cfg };      // guidance of a chain's predicted x0: chain_guide (sm_guide_host.h)

// Device data of shape guidance: per kind ONE set of groups of molecules (sm_guide_host.h installs and clears them, each in a
// DevList beside the set).  `whole`: a set of one group that spans whatever batch comes (shapemol_set_guidance /
// shapemol_set_mesh_guidance): no molecule count
struct CloudSet {     // one device block: [clouds | radii | mol_off, cloud_off, atom_off, wg_off (G + 1 ints each)]
    double *clouds = nullptr, *radius = nullptr; int *ints = nullptr;
    int groups = 0, max_points = 0, grad_step = 0; int64_t mols = 0, points = 0; bool whole = false; const double *draws = nullptr;
};
struct MeshSet {      // one device block: [faces | face boxes | clouds | bounds G x 5 | mol_off, cloud_off, atom_off, wg_off, face_off]
    MeshFace *faces = nullptr; double4 *fbox = nullptr; double *clouds = nullptr, *bounds = nullptr; int *ints = nullptr;
    int groups = 0, max_points = 0, grad_step = 0; int64_t mols = 0, nfaces = 0; bool whole = false; const double *draws = nullptr;
};

// Classifier-free guidance with one strength and one box per group of molecules (shapemol_set_cfg_groups; sm_cfg.h).  One device
// block [rows G + 1 | stat G x 2 | histograms G x 2 x kCfgHistWords] that only grows, so a captured step keeps its addresses
// from one set to the next; the tables that depend on the batch (molecule -> group, workgroups, partials) are workspace
struct CfgGroupSet {
    CfgGroup *rows = nullptr; float *stat = nullptr; unsigned *hist = nullptr; int64_t cap = 0; DevList mem;
    int groups = 0; int64_t mols = 0;
    int last_groups = 0;                                         // groups of the last chain that ran with a set (debug_read "cfg_group_stat")
    int type = 0; double p = 0.0;                                // threshold_CFG's type and p: one per chain
    float *tr_pos_u = nullptr, *tr_v_u = nullptr;                // caller's uncond trajectories (or nullptr)
    hipStream_t stream = nullptr; bool stream_set = false;      // the stream the last chain that read the rows ran on
};

// The prepared shape data one score evaluation reads (run_prep_shape writes it): invariant embedding, shape terms of layer 0
// and of every layer, VN shape part, and the argument blocks of run_prep_shape's two batched launches
struct ShapePrep { float *inv = nullptr, *add0 = nullptr, *addp = nullptr, *ps = nullptr; ShapeTermArgs *terms = nullptr; VnShapeArgs *vn = nullptr; };

}  // namespace

// Device memory (sm_devmem.h): every group of buffers is owned by the DevList declared beside its pointers, and freed with the context
struct shapemol_ctx {
    shapemol_config cfg{};
    int device = 0;
    int KP = 8;
    DevList mem_model;          // d_img, ttab, etab (shapemol_create)
    float *d_img = nullptr;
    float *ttab = nullptr;      // [T][D] time-embedding table (built once)
    float *etab = nullptr;      // [T][C][H] atom embedding of every (timestep, atom type) pair (built once)
    // the rest of the node prologue per (timestep, atom type) pair (ensure_prologue_tables; node_prologue_tab_kernel gathers from them).
    // One device block: [q_tab | pre_tab | v, mol_of, t_mol of the pseudo-batch they are built from | range flag of the build]
    float *q_tab = nullptr;     // [T][C][H] queries of layer 0's x2h attention
    float *pre_tab = nullptr;   // [T][C][4H] per-node halves of layer 0's edge MLPs, without the per-molecule term
    int64_t *tab_v = nullptr; int *tab_mol_of = nullptr, *tab_t_mol = nullptr, *tab_flag = nullptr; DevList mem_tab;
    int tab_key = 0;            // node precision mode the tables were built in (prologue_tab_key), 0 = not built
    DevModel dm;
    // workspace
    int64_t capN = 0, capB = 0;
    DevList ws{256};            // every workspace buffer: zero-filled, 256 bytes of padding behind each
    ShapePrep prep[2];          // 0: the chain's shape condition, 1: the zeroed shape of classifier-free guidance
    int *mol_of = nullptr, *mol_off = nullptr, *t_mol = nullptr, *nbr = nullptr, *steps = nullptr;
    float *temb = nullptr, *ew = nullptr;
    float *h_a = nullptr, *h_b = nullptr, *pre0 = nullptr, *preAB = nullptr, *q_x = nullptr, *q_h = nullptr, *att = nullptr, *o3 = nullptr, *pd = nullptr;
    int n_prep_terms = 0;       // shape terms of a ShapePrep (its `terms` block)
    int2 *mol_span = nullptr;   // [N] molecule span of every atom
    float *xsum = nullptr;      // [N][3] per-atom sum of the h2x attention rows (folded coordinate update)
    float *part_rows = nullptr, *part_ms = nullptr;   // k > 16: rows [2N][H] and softmax state [2N][heads][2] of the half-atom tiles
    float *alpha = nullptr;     // [N*KP][2][NT] attention weights handed from the key phase to the value phase
    float *x_a = nullptr, *x_b = nullptr, *x_state = nullptr, *pred_pos = nullptr, *pred_v = nullptr;
    int64_t *v_state = nullptr;
    unsigned long long *stamps = nullptr;   // [1024][2] diagnostic clock stamps
    unsigned long long *kstamps = nullptr;  // per-wave phase stamps of ONE selected kernel launch (SM_STAMPS build)
    int kstamp_sel = -1;                    // which launch: 0 node_pre, 1 edge_x2h, 2 edge_h2x (layer 0)
    int stamp_on = 0;
    double *bn_acc = nullptr;
    int *status = nullptr;                  // [8] sticky error flags (StatusFlag), cleared at the start of _score/_sample
    ChainParams *chain_params = nullptr;    // per-chain parameters read by the posterior-step kernel
    // last evaluation (debug_read)
    int64_t lastN = 0, lastB = 0;
    const float *last_h = nullptr, *last_x = nullptr;
    lg::Options opt;            // the options that select kernels and shape launches (sm_launch.h)
    int bn_eval = 0;            // 1: evaluation-mode batch-norm (running statistics, shapemol_set_bn_running) instead of the batch's
    DevList mem_bn;             // the two below
    float *bn_run = nullptr;    // [2][L][heads] running mean | running variance (device)
    double *bn_eval_acc = nullptr;   // [L][kVnReplicas][2][heads] sums that reproduce them for the current batch size
    DdpmFold ddpm_vf{};         // the last layer's coordinate update inside the DDPM kernel (option ddpm_fold), handed from run_score to run_ddpm
    float hid_max = 0.f;        // bound of the edge MLPs' hidden activations (LayerNorm outputs): must fit fp16 for edge_bf16 = 3
    int num_cu = 256;
    // shape guidance of the predicted x0: the installed point-cloud set and mesh set (the mesh takes precedence when both are set),
    // the per-workgroup table of whichever guides (sized by the chain) and the mesh's per-step lists (one block; counters: 4 per group)
    CloudSet cs; MeshSet ms; DevList mem_cs, mem_ms;
    int2 *wg_table = nullptr; int64_t wg_table_cap = 0; DevList mem_wg;
    // gradient shape guidance (shapemol_set_field_guidance): the borrowed decoder context, whose per-shape workspace the chain's
    // prep fills from the chain's own shapes
    shapemol_sd_ctx *field_sd = nullptr; double field_lr = 0.0; int field_step = 0;
    float4 *m_within = nullptr; int *m_out = nullptr, *m_cnt = nullptr; int64_t m_cap = 0, m_cnt_cap = 0; DevList mem_mesh;
    int64_t m_flag_groups = 0;      // groups of the last chain / pass with a mesh set (debug_read "mesh_group_flags")
    // classifier-free guidance (shapemol_set_cfg): a second score evaluation per step on a zeroed shape, whose prepared shape
    // data is prep[1] and whose outputs are pred_pos_u / pred_v_u
    double cfg_w = 0.0, cfg_p = 0.0; int cfg_type = 0, cfg_has_bounds = 0; float cfg_lo[3] = {}, cfg_hi[3] = {};
    float *cfg_tr_pos_u = nullptr, *cfg_tr_v_u = nullptr;      // caller's uncond trajectories (or nullptr)
    float *pred_pos_u = nullptr, *pred_v_u = nullptr;
    float *shape_zero = nullptr;      // [B][S][3] zeros (never written)
    float *cfg_stat = nullptr; double *cfg_part = nullptr; unsigned *cfg_hist = nullptr;
    CfgGroupSet cgs;            // per-group strengths and boxes (takes the place of the scalar form while installed)
    int *cfg_mol_grp = nullptr; int2 *cfg_blk_tab = nullptr; double *cfg_gpart = nullptr; int64_t cfg_tab_stride = 0;
    int first_step = 0;         // option "first_step": the next chains start at reverse step first_step (t = T-1-first_step)
    // diagnostic: neighbour lists pinned at given (reverse step, atom) pairs (shapemol_set_knn_pins)
    int *pin_off = nullptr, *pin_atom = nullptr, *pin_nbr = nullptr; int64_t n_pins = 0; int pin_steps = 0, pin_k = 0; DevList mem_pins;
    // profiling
    bool prof_on = false;
    std::vector<ProfRec> prof;
    hipEvent_t cur_e0 = nullptr, cur_e1 = nullptr;     // event pair of the launch being issued
    // graph cache
    hipGraphExec_t gexec = nullptr, gexec_u = nullptr;     // one step / kGraphUnroll steps
    int64_t n_captures = 0;                                // graph captures so far (debug_read "captures")
    // the launch forms the most recent run_score chose (debug_read "launch"): {sampling, fused graph kernel, a coordinate update
    // folded into an x2h kernel, the last one folded into the DDPM kernel, x2h_chain16_kernel used, streaming kernels' tiles per
    // workgroup, their grid (0, 0 on the other edge kernels), CUs}; graph_rec: those of the captured step, which a replay reports
    int64_t launch_rec[8] = {}, graph_rec[8] = {};
    // the node stage of the last layer the most recent run_score issued (debug_read "launch_node"): {two-level form used, follow-up
    // jobs, linear jobs, waves per workgroup, job order, column tiles per linear job, linear staging chunk, dynamic LDS bytes}
    int64_t node_rec[8] = {};
    // the x2h kernel's fused tail in that layer (debug_read "launch_x2h_out"): {fused form used, atoms per workgroup, 16-atom column
    // tiles per workgroup, dynamic LDS bytes of the x2h launch}
    int64_t x2h_out_rec[4] = {};
    // the edge tiles of that evaluation (debug_read "launch_edge"): {half-atom tiles used (k > 16), tiles per attention, combine32_kernel
    // launches issued, floats of a part_rows row}
    int64_t edge_rec[4] = {};
    // the captured step depends on the batch geometry only: seed, noise and trajectory pointers live in chain_params
    // what a captured step depends on besides the options (which drop the graphs when set): sizes, guidance, and the two
    // launch decisions taken from the max_mol_atoms hint (folded coordinate update, fused graph kernel)
    // (classifier-free guidance: its type and scalars are kernel arguments of the captured step)
    struct GraphKey { int64_t N = 0, B = 0; Guide guide = Guide::None; int fold = 0, gfuse = 0;
                      int cfg = 0 /* 0 off, else 1 + CfgType */; double cfgv[9] = {};   // w, p, has_bounds, box
                      int cfg_groups = 0;     // groups of the per-group form (its strengths, boxes and layout live in device memory), else 0
                      // field guidance: the never-reused identity of the decoder's device memory (the step holds the addresses of its
                      // weights and workspace; 0 = no field), grad_lr, grad_step
                      uint64_t field_gen = 0; double field_lr = 0.0; int field_step = 0;
                      bool operator==(const GraphKey &o) const {
                          if (!(N == o.N && B == o.B && guide == o.guide && fold == o.fold && gfuse == o.gfuse && cfg == o.cfg &&
                                cfg_groups == o.cfg_groups && field_gen == o.field_gen && field_lr == o.field_lr &&
                                field_step == o.field_step)) return false;
                          for (int i = 0; i < 9; ++i) if (cfgv[i] != o.cfgv[i]) return false;
                          return true;
                      } } gkey{};
    hipStream_t gstream = nullptr; bool gstream_set = false;     // the stream the executables were last launched on
    void drop_graphs() {      // a replay may still be in flight: drain it before destroying the executables (only the stream the
        if (!gexec && !gexec_u) return;       // graphs ran on: another context's chain may be running beside, and must not be waited for)
        if (!gstream_set || hipStreamSynchronize(gstream) != hipSuccess) hipDeviceSynchronize();
        if (gexec) { hipGraphExecDestroy(gexec); gexec = nullptr; }
        if (gexec_u) { hipGraphExecDestroy(gexec_u); gexec_u = nullptr; }
    }
    const float *P(size_t off) const { return d_img + off; }
};

namespace {

// Profiling mode (shapemol_profile_begin): every kernel is launched with hipExtLaunchKernelGGL and a start/stop event
// pair that takes the begin/end timestamps of the DISPATCH ITSELF (what rocprofv3's kernel trace reports), not of
// marker packets around it.
#define SMK(kern, grid, block, shm, stream, ...)                                                                    \
    do {                                                                                                             \
        if (c->prof_on) hipExtLaunchKernelGGL(kern, grid, block, shm, stream, c->cur_e0, c->cur_e1, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, block, shm, stream, __VA_ARGS__);                                        \
    } while (0)

template <typename F>
int launch(shapemol_ctx *c, const char *name, hipStream_t s, F &&f) {
    (void)s;
    if (c->prof_on) {
        ProfRec r{name, nullptr, nullptr};
        HIPCHK(hipEventCreate(&r.e0)); HIPCHK(hipEventCreate(&r.e1));
        c->cur_e0 = r.e0; c->cur_e1 = r.e1;
        f();
        c->prof.push_back(r);
    } else {
        f();
    }
    HIPCHK(hipGetLastError());
    return 0;
}
#define LAUNCH(name, ...) do { if (launch(c, name, s, [&]() { __VA_ARGS__; })) return 1; } while (0)

// The workspace buffers for capN atoms in capB molecules, into the released list c->ws: one allocation per buffer, in this order
int workspace_alloc(shapemol_ctx *c, int64_t capN, int64_t capB) {
    const shapemol_config &g = c->cfg;
    const int H = g.hidden_dim, L = g.num_layers, hd = g.n_heads;
    hipError_t e = hipSuccess;
    auto A = [&](auto **p, size_t n) -> int { return (e = c->ws.alloc(p, n * sizeof(**p), true)) != hipSuccess; };
    auto prep_data = [&](ShapePrep &p) -> int {
        return A(&p.inv, capB * g.shape_latent_dim) || A(&p.add0, (size_t)capB * 4 * H) || A(&p.addp, (size_t)L * capB * 8 * H) || A(&p.ps, (size_t)L * capB * 2 * hd * 3);
    };
    auto prep_args = [&](ShapePrep &p) -> int { return A(&p.terms, 2 * L + 1) || A(&p.vn, L); };
    // per-group classifier-free guidance: workgroup tables and partials for the largest launch bound of this capacity
    // (elements / 2048 + groups per tensor, cfg_group_blocks), molecule -> group
    const int64_t stride = capN * std::max(g.num_classes, 3) / 2048 + kCfgMaxGroups + 1;
    if (A(&c->mol_of, capN) || A(&c->mol_off, capB + 1) || A(&c->t_mol, capB) || A(&c->nbr, capN * c->KP) ||
        A(&c->steps, 4) || A(&c->temb, capB * g.time_emb_dim) || prep_data(c->prep[0]) || A(&c->ew, capN * c->KP) ||
        A(&c->h_a, capN * H) || A(&c->h_b, capN * H) || A(&c->pre0, capN * 4 * H) || A(&c->preAB, capN * 8 * H) || A(&c->q_x, capN * H) || A(&c->q_h, capN * H) ||
        A(&c->att, capN * H) || A(&c->o3, capN * 48) || A(&c->xsum, capN * 3) || A(&c->mol_span, capN) || A(&c->alpha, capN * c->KP * 2 * (H / 16)) || A(&c->pd, capN * hd * 6) || A(&c->x_a, capN * 3) ||
        A(&c->x_b, capN * 3) || A(&c->x_state, capN * 3) || A(&c->pred_pos, capN * 3) ||
        A(&c->pred_v, capN * g.num_classes) || A(&c->v_state, capN) || A(&c->stamps, 2048) || A(&c->kstamps, 8 * 16 * 4096) || A(&c->bn_acc, (size_t)L * kVnReplicas * 2 * hd + L + 1) ||
        (c->KP > 16 && (A(&c->part_rows, (size_t)2 * capN * H) || A(&c->part_ms, (size_t)2 * capN * hd * 2))) ||
        A(&c->status, 8) || A(&c->chain_params, 1) || prep_args(c->prep[0]) ||
        prep_data(c->prep[1]) || A(&c->pred_pos_u, capN * 3) || A(&c->pred_v_u, capN * g.num_classes) ||
        A(&c->shape_zero, (size_t)capB * g.shape_dim * 3) || prep_args(c->prep[1]) ||
        A(&c->cfg_stat, 4) || A(&c->cfg_part, (size_t)2 * kCfgMaxBlocks * 4) || A(&c->cfg_hist, (size_t)2 * kCfgHistWords) ||
        A(&c->cfg_mol_grp, capB) || A(&c->cfg_blk_tab, (size_t)2 * stride) || A(&c->cfg_gpart, (size_t)2 * stride * 4))
        return hip_fail("workspace allocation", e);
    c->cfg_tab_stride = stride;
    // argument blocks of the batched prep launches (they point into the workspace just allocated), one per set of shape data
    for (ShapePrep &p : c->prep) {
        const int SL = g.shape_latent_dim, S = g.shape_dim;
        std::vector<ShapeTermArgs> terms;
        std::vector<VnShapeArgs> vns;
        const DevLayer &D0 = c->dm.layer[0];
        terms.push_back(ShapeTermArgs{p.inv, c->P(D0.sk_x2h), c->P(D0.bk_x2h), c->P(D0.sv_x2h), c->P(D0.bv_x2h), p.add0, SL, H, SL, 4 * H});
        for (int l = 0; l < L; ++l) {
            const DevLayer &D = c->dm.layer[l];
            float *addp = p.addp + (size_t)l * capB * 8 * H;      // [B][8H]: this layer's h2x | the next layer's x2h
            terms.push_back(ShapeTermArgs{p.inv, c->P(D.sk_h2x), c->P(D.bk_h2x), c->P(D.sv_h2x), c->P(D.bv_h2x), addp, SL, H, SL, 8 * H});
            if (l + 1 < L) {
                const DevLayer &Dn = c->dm.layer[l + 1];
                terms.push_back(ShapeTermArgs{p.inv, c->P(Dn.sk_x2h), c->P(Dn.bk_x2h), c->P(Dn.sv_x2h), c->P(Dn.bv_x2h), addp + 4 * H, SL, H, SL, 8 * H});
            }
            vns.push_back(VnShapeArgs{nullptr, c->P(D.vn_f), c->P(D.vn_d), p.ps + (size_t)l * capB * 2 * hd * 3, S, hd});
        }
        c->n_prep_terms = (int)terms.size();
        HIPCHK(hipMemcpy(p.terms, terms.data(), terms.size() * sizeof(ShapeTermArgs), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p.vn, vns.data(), vns.size() * sizeof(VnShapeArgs), hipMemcpyHostToDevice));
    }
    return 0;
}

// The workspace only grows.  While it is rebuilt the context has none: capacities 0, every workspace pointer null (the list's
// release), nothing of a last evaluation to read and no captured step -- which is also the state a failed growth leaves
int ensure_workspace(shapemol_ctx *c, int64_t N, int64_t B) {
    if (N <= c->capN && B <= c->capB) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    c->drop_graphs();
    const int64_t capN = std::max<int64_t>(N, c->capN), capB = std::max<int64_t>(B, c->capB);
    c->ws.release();
    c->capN = c->capB = 0; c->lastN = c->lastB = 0; c->last_h = c->last_x = nullptr;
    if (workspace_alloc(c, capN, capB)) { c->ws.release(); return 1; }
    c->capN = capN; c->capB = capB;
    return 0;
}

}  // namespace

#include "sm_guide_host.h"

namespace {

constexpr int kVnFoldBytes = kVnFoldCap * 3 * 4 + 32 * 8;      // LDS of the folded coordinate update: table + batch sums

// What sm_launch.h computes every launch geometry and step form from: the options, the kernel headers' constants, the sizes
template <int H>
lg::In launch_in(const shapemol_ctx *c, int n_atoms) {
    constexpr bool chain16_fits = Chain16Lds<H>::BYTES <= 2 * EdgeImage16<H, H / 16>::TOTAL * 4;
    return {c->opt, {kVnFoldCap, kStreamTPR, CHAIN_COLS, kGraphCap, kLin6Chunk, chain16_fits}, c->KP, c->num_cu, H, n_atoms};
}

// Largest dynamic LDS of every kernel that needs more than the default: one size per kernel family
#define ATTR(bytes, ...) HIPCHK(hipFuncSetAttribute((const void *)__VA_ARGS__, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)))
template <int H, int K>
int set_edge_attr_k() {
    constexpr int NT = H / 16;
    constexpr int vn_tail = vn_red_doubles(12, H / 8) * 8 + 12 * 96 * 4;     // h2x, 12 waves: reduction scratch + attention rows of the fused coordinate update
    constexpr int fold = K <= 16 ? kVnFoldBytes : 0;                         // x2h: table of the folded coordinate update (not for k > 16)
    constexpr int x16 = 2 * EdgeImage16<H, NT>::TOTAL * 4 + fold, h16 = (EdgeImage16<H, NT>::TOTAL + EdgeImage16<H, 1>::TOTAL) * 4 + vn_tail;
    ATTR(x16, edge16_kernel<H, K, false>); ATTR(x16, edge16_kernel<H, K, false, true>);
    ATTR(x16, edge16_loop_kernel<H, K, false>); ATTR(x16, edge16_loop_kernel<H, K, false, true>);
    ATTR(h16, edge16_kernel<H, K, true>); ATTR(h16, edge16_kernel<H, K, true, true>);
    ATTR(h16, edge16_loop_kernel<H, K, true>); ATTR(h16, edge16_loop_kernel<H, K, true, true>);
    ATTR((StreamMap<H, false>::O_TAIL * 4 + kVnFoldBytes), edge_stream_kernel<H, K, false>);
    ATTR((StreamMap<H, true>::O_TAIL * 4 + (NT + kStreamProducers) * 64 * 2 * 8), edge_stream_kernel<H, K, true>);
    if constexpr (K <= 16) {      // kernels of single-tile jobs only
        constexpr int xph = EdgePhaseImage<H, NT>::TOTAL * 4, hph = (EdgePhaseImage<H, NT>::TOTAL + EdgePhaseImage<H, 1>::TOTAL) * 4 + vn_tail;
        ATTR(x16, x2h_chain16_kernel<H, K>); ATTR(x16, x2h_chain16_kernel<H, K, true>);
        ATTR((EdgeBlob<H, false>::TOTAL * 4), edge_attention_kernel<H, K, false>); ATTR((EdgeBlob<H, true>::TOTAL * 4), edge_attention_kernel<H, K, true>);
        ATTR(xph, edge_fused_kernel<H, K, false, false>); ATTR(xph, edge_fused_kernel<H, K, false, true>);
        ATTR(hph, edge_fused_kernel<H, K, true, false>); ATTR(hph, edge_fused_kernel<H, K, true, true>);
    }
    return 0;
}

template <int H>
int set_edge_attr(int KP) {
    constexpr size_t pro16 = Prologue16Lds<H>::BYTES;
    ATTR(Prologue6Lds<H>::BYTES, node_prologue6_kernel<H>); ATTR(Chain6Lds<H>::BYTES, node_chain6_kernel<H>); ATTR(kLin6Chunk * 3 * H * 32, node_linear6_kernel<H>);
    ATTR(Out6Lds<H>::BYTES, node_out6_kernel<H>); ATTR(After6Lds<H>::bytes(kLin6Chunk), node_after6_kernel<H>);
    ATTR(pro16, node_prologue16_kernel<H>); ATTR(Chain16Lds<H>::BYTES, node_chain16_kernel<H>); ATTR(kLin16Chunk * 2 * H * 32, node_linear16_kernel<H>);
    ATTR(pro16, node_prologue16_kernel<H, true>); ATTR(Chain16Lds<H>::BYTES, node_chain16_kernel<H, true>); ATTR(kLin16Chunk * 2 * H * 32, node_linear16_kernel<H, true>);
    return KP == 8 ? set_edge_attr_k<H, 8>() : (KP == 16 ? set_edge_attr_k<H, 16>() : set_edge_attr_k<H, 32>());
}
#undef ATTR

// One launch of KERNEL<H, KP TAIL> for the context's padded neighbour count: TAIL = (, further template arguments) or ().
// DISPATCH_KP16: kernels of single-tile jobs, not instantiated for k > 16 (the caller has ruled it out); _F16: kernels with a
// trailing "f16 features" flag (option feat_f16)
#define SM_ARGS(...) __VA_ARGS__
#define LAUNCH_KP(name, K, KERNEL, TAIL, ...) LAUNCH(name, SMK((KERNEL<H, K SM_ARGS TAIL>), __VA_ARGS__))
#define DISPATCH_KP16(name, KERNEL, TAIL, ...)                                                      \
    do { if (KP == 8) LAUNCH_KP(name, 8, KERNEL, TAIL, __VA_ARGS__); else LAUNCH_KP(name, 16, KERNEL, TAIL, __VA_ARGS__); } while (0)
#define DISPATCH_KP(name, KERNEL, TAIL, ...)                                                        \
    do { if (KP > 16) LAUNCH_KP(name, 32, KERNEL, TAIL, __VA_ARGS__); else DISPATCH_KP16(name, KERNEL, TAIL, __VA_ARGS__); } while (0)
#define DISPATCH_KP_F16(DISPATCH, name, KERNEL, TAIL, ...)                                          \
    do { if (c->opt.feat_f16) DISPATCH(name, KERNEL, (SM_ARGS TAIL, true), __VA_ARGS__); else DISPATCH(name, KERNEL, TAIL, __VA_ARGS__); } while (0)

template <int H, bool H2X>
int launch_edge(shapemol_ctx *c, hipStream_t s, const EdgeArgs &a) {     // fp32-MFMA edge kernel (option edge_bf16 = 0; k > 16)
    const int KP = c->KP;
    const lg::EdgeGeom g = lg::edge_fp32_geom(launch_in<H>(c, a.n_atoms));
    const size_t shm = EdgeBlob<H, H2X>::TOTAL * sizeof(float);
    const char *nm = H2X ? "edge_h2x" : "edge_x2h";
    if (KP > 16) return fail("k > 16 runs on the two-piece f16 edge kernels only (option edge_bf16 = 3)");
    DISPATCH_KP16(nm, edge_attention_kernel, (, H2X), dim3(g.grid), dim3(g.waves * 64), shm, s, a);
    return 0;
}

template <int H, bool H2X>
int launch_fused(shapemol_ctx *c, hipStream_t s, const EdgeFusedArgs &a) {
    const int KP = c->KP;
    const lg::EdgeGeom g = lg::edge_phase_geom(launch_in<H>(c, a.n_atoms));
    const size_t shm = (EdgePhaseImage<H, H / 16>::TOTAL + (H2X ? EdgePhaseImage<H, 1>::TOTAL : 0)) * sizeof(float)
                       + (H2X ? (size_t)vn_red_doubles(g.waves, H / 8) * 8 + (size_t)g.waves * g.apj * 48 * 4 : 0);   // + reduction scratch and attention rows of the fused coordinate update
    const char *nm = H2X ? "edge_h2x" : "edge_x2h";
    if (g.form == lg::Form::One) DISPATCH_KP16(nm, edge_fused_kernel, (, H2X, true), dim3(g.grid), dim3(g.waves * 64), shm, s, a);      // straight-line instantiation
    else DISPATCH_KP16(nm, edge_fused_kernel, (, H2X, false), dim3(g.grid), dim3(g.waves * 64), shm, s, a);
    return 0;
}

template <int H, bool H2X>
int launch_edge16(shapemol_ctx *c, hipStream_t s, const Edge16Args &a) {
    const int KP = c->KP;
    const char *nm = H2X ? "edge_h2x" : "edge_x2h";
    const lg::EdgeGeom g = lg::edge16_geom(launch_in<H>(c, a.n_atoms));
    const size_t shm = (EdgeImage16<H, H / 16>::TOTAL + EdgeImage16<H, (H2X ? 1 : H / 16)>::TOTAL) * sizeof(float)
                       + (H2X ? (size_t)vn_red_doubles(g.waves, H / 8) * 8 + (size_t)g.waves * g.apj * 48 * 4 : (a.vf.enable ? kVnFoldBytes : 0));
    Edge16Args b = a;
    b.nwave = g.waves;
    if (g.form == lg::Form::Loop) {      // every workgroup owns `chunk` consecutive jobs
        b.job_base = 0; b.job_end = g.jobs; b.chunk = g.chunk;
        DISPATCH_KP_F16(DISPATCH_KP, nm, edge16_loop_kernel, (, H2X), dim3(g.grid), dim3(g.waves * 64), shm, s, b);
        return 0;
    }
    // one launch of the straight-line instantiation, or (larger batches, edge_tiles = 0) several, each over a slice of the jobs
    for (int base = 0; base < g.jobs; base += g.slice) {
        b.job_base = base; b.job_end = std::min(g.jobs, base + g.slice);
        DISPATCH_KP_F16(DISPATCH_KP, nm, edge16_kernel, (, H2X), dim3(lg::slice_grid(g, base)), dim3(g.waves * 64), shm, s, b);
    }
    return 0;
}

template <int H, bool H2X>
int launch_stream(shapemol_ctx *c, hipStream_t s, EdgeStreamArgs a) {      // streaming edge kernels (sm_edge_stream.h; option edge_bf16 = 2)
    const int KP = c->KP;
    const lg::StreamGeom g = lg::stream_geom(launch_in<H>(c, a.n_atoms));
    a.chunk = g.chunk;
    using M = StreamMap<H, H2X>;
    constexpr int NWAVE = H / 16 + kStreamProducers;
    const size_t shm = (size_t)M::O_TAIL * 4 + (H2X ? (size_t)NWAVE * 64 * 2 * 8 : (a.vf.enable ? (size_t)kVnFoldBytes : 0));
    const char *nm = H2X ? "edge_h2x" : "edge_x2h";
    if (!H2X) {
        const int64_t rec[4] = {a.no.h_out != nullptr, g.atoms_per_wg, (g.atoms_per_wg + 15) / 16, (int64_t)shm};
        std::copy(rec, rec + 4, c->x2h_out_rec);
    }
    DISPATCH_KP(nm, edge_stream_kernel, (, H2X), dim3(g.grid), dim3(NWAVE * 64), shm, s, a);
    return 0;
}

// k > 16: merge the two half-atom tiles of every atom (combine32_kernel) into `out` ([N][H] or [N][48])
template <bool H2X>
int launch_combine32(shapemol_ctx *c, hipStream_t s, float *out, int n_atoms) {
    Combine32Args ca{c->part_rows, c->part_ms, out, n_atoms, c->cfg.n_heads, c->cfg.hidden_dim / 16};
    const int items = n_atoms * (H2X ? 48 : c->cfg.hidden_dim / 4);
    ++c->edge_rec[2];
    LAUNCH("edge_combine", SMK(combine32_kernel<H2X>, dim3((items + 255) / 256), dim3(256), 0, s, ca));
    return 0;
}

template <int H>
int launch_x2h_chain(shapemol_ctx *c, hipStream_t s, const Edge16Args &a, const NodeChainArgs &na) {      // x2h attention + node stage in one launch
    const int KP = c->KP;
    const lg::EdgeGeom g = lg::x2h_chain_geom(launch_in<H>(c, a.n_atoms));
    const size_t shm = 2 * EdgeImage16<H, H / 16>::TOTAL * sizeof(float) + (a.vf.enable ? kVnFoldBytes : 0);
    Edge16Args b = a;
    b.job_base = 0; b.job_end = g.jobs; b.nwave = g.waves;
    DISPATCH_KP_F16(DISPATCH_KP16, "edge_x2h_chain", x2h_chain16_kernel, (), dim3(g.grid), dim3(g.waves * 64), shm, s, b, na, c->status + ST_RANGE);
    return 0;
}

template <int H, int KT>
int launch_mlp2(shapemol_ctx *c, hipStream_t s, const char *name, const DevMlpImg &m, const float *in0, const float *in1,
                int mode, const float *resid, float *out, int ld_out, int n_store, int n_atoms) {
    NodeMlpArgs a{};
    a.in0 = in0; a.in1 = in1; a.w1img = c->P(m.w1img); a.b1 = c->P(m.b1); a.ln_g = c->P(m.g); a.ln_b = c->P(m.be);
    a.w2img = c->P(m.w2img); a.b2 = c->P(m.b2); a.resid = resid; a.out = out; a.ld_out = ld_out; a.n_store = n_store;
    a.mode = mode; a.nt2 = m.nt2; a.n_atoms = n_atoms;
    const int n_ct = (n_atoms + 15) / 16, teams = NodeMlpLds<H>::TEAMS;
    LAUNCH(name, SMK((node_mlp2_kernel<H, KT>), dim3((n_ct + teams - 1) / teams), dim3(kNodeThreads), 0, s, a));
    return 0;
}

template <int H>
int launch_linear(shapemol_ctx *c, hipStream_t s, const char *name, const float *in, const float *wimg, const float *wimg6, const float *wimg16, const float *add_mol,
                  int ld_add, float *out, int ld_out, int n_out_tiles, int n_atoms, unsigned long long *stamps) {
    const lg::LinGeom g = lg::linear_geom(launch_in<H>(c, n_atoms), n_out_tiles);
    const dim3 grid(g.ogroups * g.agroups), block(g.waves * 64);
    const bool f16 = c->opt.lin_bf16 && c->opt.node_f16;
    NodeLinArgs a{in, f16 ? wimg16 : (c->opt.lin_bf16 ? wimg6 : wimg), add_mol, c->mol_of, out, n_atoms, n_out_tiles, g.tpg, ld_add, ld_out, stamps, g.waves};
    if (f16) {
        const size_t shm = (size_t)std::min(g.tpg, kLin16Chunk) * 2 * H * 32;
        if (c->opt.feat_f16) LAUNCH(name, SMK((node_linear16_kernel<H, true>), grid, block, shm, s, a, c->status + ST_RANGE));
        else LAUNCH(name, SMK(node_linear16_kernel<H>, grid, block, shm, s, a, c->status + ST_RANGE));
    } else if (c->opt.lin_bf16) {
        const size_t shm = (size_t)std::min(g.tpg, kLin6Chunk) * 3 * H * 32;
        LAUNCH(name, SMK(node_linear6_kernel<H>, grid, block, shm, s, a));
    } else {
        LAUNCH(name, SMK(node_linear_kernel<H>, grid, block, 0, s, a));
    }
    return 0;
}

// The exact-mode node stage in two dependency levels: h' (node_out6_kernel), then the follow-up MLPs and the per-node products of h'
// in one launch (node_after6_kernel).  na as for node_chain6_kernel; the products as launch_linear would compute them.
template <int H>
int launch_node_levels(shapemol_ctx *c, hipStream_t s, const NodeChainArgs &na, const float *lin_img6, const float *add_mol, int ld_add,
                       float *out, int ld_out, int lin_tiles, bool out_done) {
    const int n = na.n_atoms;
    const lg::NodeLevelsGeom g = lg::node_levels_geom(launch_in<H>(c, n), na.n_follow, lin_tiles);
    if (!out_done) LAUNCH("node_chain", SMK(node_out6_kernel<H>, dim3(g.n_pairs), dim3(H * 4), Out6Lds<H>::BYTES, s, na));      // (else: the x2h kernel's tail wrote h')
    NodeAfterArgs a{};
    a.f[0] = na.f[0]; a.f[1] = na.f[1];
    a.n_pairs = g.n_pairs; a.n_fjobs = g.n_fjobs; a.n_ljobs = g.n_ljobs; a.order = c->opt.after_order; a.lin_chunk = g.lin_chunk;
    a.lin = NodeLinArgs{na.h_out, lin_img6, add_mol, c->mol_of, out, n, lin_tiles, g.tpg, ld_add, ld_out, nullptr, g.lw};
    const size_t shm = After6Lds<H>::bytes(a.lin_chunk);
    const int64_t rec[8] = {1, a.n_fjobs, a.n_ljobs, g.bw, a.order, g.tpg, a.lin_chunk, (int64_t)shm};
    std::copy(rec, rec + 8, c->node_rec);
    LAUNCH("node_pre", SMK(node_after6_kernel<H>, dim3(a.n_fjobs + a.n_ljobs), dim3(g.bw * 64), shm, s, a));
    return 0;
}

NodeFollow follow_of(const shapemol_ctx *c, const DevMlpImg &m, int mode, float *out, int ld_out, int n_store) {
    NodeFollow f{};
    f.w1img = c->P(m.w1img); f.b1 = c->P(m.b1); f.ln_g = c->P(m.g); f.ln_b = c->P(m.be);
    f.w1img6 = c->P(c->opt.node_f16 ? m.w1img16 : m.w1img6); f.w2img6 = c->P(c->opt.node_f16 ? m.w2img16 : m.w2img6);
    f.w2img = c->P(m.w2img); f.b2 = c->P(m.b2); f.out = out; f.ld_out = ld_out; f.n_store = n_store; f.mode = mode; f.nt2 = m.nt2;
    return f;
}

// Step-invariant per-batch quantities (molecule index, invariant shape embedding, shape terms)
// Diagnostic (shapemol_set_knn_pins): overwrite the neighbour rows of the atoms pinned at the current reverse step with the
// given lists.  off [steps + 1] CSR offsets per reverse step, atom [n], pnbr [n][k].
__global__ void knn_pin_kernel(const int *off, int n_steps, const int *atom, const int *pnbr, int k, int kp, const int *step_cur, int n_atoms, int *nbr) {
    const int step = *step_cur;
    if (step < 0 || step >= n_steps) return;
    const int lo = off[step], hi = off[step + 1];
    for (int e = lo + blockIdx.x * blockDim.x + threadIdx.x; e < hi; e += gridDim.x * blockDim.x) {
        const int i = atom[e];
        if (i < 0 || i >= n_atoms) continue;
        for (int sl = 0; sl < kp; ++sl) nbr[(size_t)i * kp + sl] = sl < k ? pnbr[(size_t)e * k + sl] : -1;
    }
}

template <int H>
int run_prep_shape(shapemol_ctx *c, hipStream_t s, int64_t B, const float *d_shape, const ShapePrep &sp);

// the launch bound of the per-group statistic kernels for a tensor of n elements: the sum over the groups of
// min(kCfgMaxBlocks, max(1, ceil(n_g / 2048))) is at most n / 2048 + G
int cfg_group_blocks(int64_t n, int n_groups) { return (int)(n / 2048 + n_groups); }

CfgArgs cfg_args(const shapemol_ctx *c, int64_t N) {
    CfgArgs a{};
    a.on = chain_guide(c) == Guide::Cfg ? 1 : 0;
    if (!a.on) return a;
    const int C = c->cfg.num_classes;
    a.pos_c = c->pred_pos; a.pos_u = c->pred_pos_u; a.v_c = c->pred_v; a.v_u = c->pred_v_u;
    if (c->cgs.groups > 0) {      // per group: strengths, boxes, ranges and ranks are the rows' (device memory)
        a.pf = (float)c->cgs.p; a.qf = (float)(1.0 - c->cgs.p); a.type = c->cgs.type; a.n_atoms = (int)N; a.C = C;
        a.stat = c->cgs.stat; a.part = c->cfg_gpart; a.hist = c->cgs.hist;
        a.grp = c->cgs.rows; a.mol_grp = c->cfg_mol_grp; a.blk_tab = c->cfg_blk_tab;
        a.n_groups = c->cgs.groups; a.tab_stride = (int)c->cfg_tab_stride;
        for (int w = 0; w < 2; ++w) a.blocks[w] = cfg_group_blocks(N * (w ? C : 3), c->cgs.groups);
        return a;
    }
    a.w1 = (float)(1.0 + c->cfg_w); a.w = (float)c->cfg_w; a.pf = (float)c->cfg_p; a.qf = (float)(1.0 - c->cfg_p);
    for (int k = 0; k < 3; ++k) { a.lo[k] = c->cfg_lo[k]; a.hi[k] = c->cfg_hi[k]; }
    a.has_bounds = c->cfg_has_bounds; a.type = c->cfg_type; a.n_atoms = (int)N; a.C = C;
    a.stat = c->cfg_stat; a.part = c->cfg_part; a.hist = c->cfg_hist;
    for (int w = 0; w < 2; ++w) {
        const int64_t n = N * (w ? C : 3);
        a.blocks[w] = (int)std::min<int64_t>(kCfgMaxBlocks, std::max<int64_t>(1, (n + 2047) / 2048));
        // torch.quantile: q rounded to float32, rank = q * (n - 1) in float32, the two ranks around it, weight rank - below
        volatile float q = (float)c->cfg_p, last = (float)(n - 1);
        volatile float rank = q * last;
        a.k_lo[w] = (long long)rank;
        a.k_hi[w] = (long long)std::ceil(rank);
        a.weight[w] = rank - (float)a.k_lo[w];
        a.k_lo[w] = std::min<long long>(std::max<long long>(a.k_lo[w], 0), n - 1);
        a.k_hi[w] = std::min<long long>(std::max<long long>(a.k_hi[w], 0), n - 1);
    }
    return a;
}

// classifier-free guidance, after both score evaluations: the batch statistic of each tensor (threshold_CFG's s or r)
int run_cfg_stats(shapemol_ctx *c, hipStream_t s, const CfgArgs &a) {
    const dim3 grid((unsigned)std::max(a.blocks[0], a.blocks[1]), 2);
    if (a.type == CFG_REFERENCE || a.type == CFG_RESCALE) {
        LAUNCH("cfg_stat", SMK(cfg_partial_kernel, grid, dim3(256), 0, s, a));
    } else if (a.type == CFG_DYNAMIC) {
        LAUNCH("cfg_stat", SMK(cfg_hist_kernel<0>, grid, dim3(256), 0, s, a));
        LAUNCH("cfg_stat", SMK(cfg_hist_kernel<1>, grid, dim3(256), 0, s, a));
        LAUNCH("cfg_stat", SMK(cfg_hist_kernel<2>, grid, dim3(256), 0, s, a));
    } else {
        return 0;        // no threshold: the combine and the clamp need no statistic
    }
    LAUNCH("cfg_stat", SMK(cfg_finalize_kernel, dim3(2, a.grp ? a.n_groups : 1), dim3(256), 0, s, a));
    return 0;
}

// classifier-free guidance, once per chain (and per shapemol_debug_cfg_stats call) before the first statistic stage: cleared
// histograms and, with groups, their element ranges, workgroups and ranks from the batch vector
int run_cfg_prep(shapemol_ctx *c, hipStream_t s, const int64_t *d_batch, int64_t N, int64_t B) {
    HIPCHK(hipMemsetAsync(c->cfg_hist, 0, (size_t)2 * kCfgHistWords * sizeof(unsigned), s));
    if (c->cgs.groups > 0) {
        const CfgArgs ca = cfg_args(c, N);
        HIPCHK(hipMemsetAsync(c->cgs.hist, 0, (size_t)c->cgs.groups * 2 * kCfgHistWords * sizeof(unsigned), s));
        LAUNCH("prep", SMK(cfg_groups_table_kernel, dim3(1), dim3(256), 0, s, d_batch, (int)N, ca.C, ca.n_groups, (int)B, ca.pf, c->cgs.rows,
                           c->cfg_mol_grp, c->cfg_blk_tab, ca.tab_stride, ca.blocks[0], ca.blocks[1]));
        c->cgs.stream = s; c->cgs.stream_set = true; c->cgs.last_groups = c->cgs.groups;
    }
    return 0;
}

template <int H>
int run_prep(shapemol_ctx *c, hipStream_t s, const int64_t *d_batch, int64_t N, int64_t B, const float *d_shape, const ShapePrep &sp) {
    LAUNCH("prep", SMK(mol_index_kernel, dim3((N + 255) / 256), dim3(256), 0, s, d_batch, (int)N, (int)B, c->mol_of, c->mol_off, c->status));
    LAUNCH("prep", SMK(mol_span_kernel, dim3((N + 255) / 256), dim3(256), 0, s, c->mol_of, c->mol_off, (int)N, c->mol_span));
    return run_prep_shape<H>(c, s, B, d_shape, sp);
}

// the shape-dependent part of run_prep, into the set sp
template <int H>
int run_prep_shape(shapemol_ctx *c, hipStream_t s, int64_t B, const float *d_shape, const ShapePrep &sp) {
    const shapemol_config &g = c->cfg;
    const int L = g.num_layers, SL = g.shape_latent_dim, S = g.shape_dim;
    ShapeInvArgs si{d_shape, c->P(c->dm.inv.w1), c->P(c->dm.inv.b1), c->P(c->dm.inv.g), c->P(c->dm.inv.be),
                    c->P(c->dm.inv.w2), c->P(c->dm.inv.b2), sp.inv, S, SL};
    LAUNCH("prep", SMK(shape_invariant_kernel, dim3(B), dim3(64), 0, s, si));
    // every step-invariant shape term (layer-0 x2h; per layer h2x | next x2h) and the shape part of every VN-linear: two launches
    if (SL == 32) LAUNCH("prep", SMK(shape_term_multi_tiled_kernel<32>, dim3((unsigned)((B + kShapeTermMols - 1) / kShapeTermMols), (unsigned)c->n_prep_terms), dim3(256), 0, s, sp.terms, (int)B));
    else LAUNCH("prep", SMK(shape_term_multi_kernel, dim3((unsigned)B, (unsigned)c->n_prep_terms), dim3(256), 0, s, sp.terms));
    LAUNCH("prep", SMK(vn_shape_multi_kernel, dim3((unsigned)B, (unsigned)L), dim3(128), 0, s, d_shape, sp.vn));
    return 0;
}

// the fields Edge16Args and EdgeStreamArgs share (they use the same member names on purpose)
template <typename A>
void fill_edge(A &a, const shapemol_ctx *c, const float *pre, int ld_pre, const float *q, const float *x, float *out, int n_atoms,
               bool half_tiles, unsigned long long *stamps) {
    a.pre = pre; a.ld_pre = ld_pre; a.q = q; a.x = x; a.nbr = c->nbr; a.ew = c->ew; a.out = out; a.n_atoms = n_atoms; a.stamps = stamps;
    if (half_tiles) { a.out = c->part_rows; a.part_ms = c->part_ms; }       // k > 16: per-tile rows, merged by combine32_kernel
}

// VN-linear + batch statistics (enable = 2) or the whole coordinate update (1) of layer l behind its h2x attention
EdgeFusedArgs::VnFuse vn_fuse_args(const shapemol_ctx *c, const ShapePrep &sp, int l, float *x_next, unsigned *arrive, int enable) {
    const DevLayer &D = c->dm.layer[l];
    const int hd = c->cfg.n_heads;
    return {sp.ps + (size_t)l * c->capB * 2 * hd * 3, c->P(D.wf_x), c->P(D.wd_x), c->P(D.wf_o), c->P(D.wd_o), c->P(D.bn_g), c->P(D.bn_b),
            c->mol_of, c->pd, c->bn_acc + (size_t)l * kVnReplicas * 2 * hd, arrive, c->status + ST_VN_BARRIER, x_next, enable};
}

// What follows the h2x attention of layer l on the f16 / streaming kernels (vn_fuse = 0 or 2): the VN-linear + statistics epilogue
// (not on half-atom tiles), and who finishes the coordinate update -- the next layer's x2h kernel (`pending`), the DDPM kernel
// (`ddpm`: the model's last layer in a chain step whose predicted x0 nobody reads before: no guidance, no CFG), or, with neither,
// the vn_apply launch (vn_done = false; vn_stats too unless stats_done)
struct H2xPlan { EdgeFusedArgs::VnFuse vn{}; float *xsum = nullptr; VnFold pending{}; DdpmFold ddpm{}; bool stats_done = false, vn_done = false; };
H2xPlan h2x_plan(const shapemol_ctx *c, const ShapePrep &sp, int l, bool fold, bool has_next, bool half_tiles, const double *stat_acc, const float *cur_x,
                 float *x_next, float *out_pos) {
    H2xPlan p;
    if (!c->opt.vn_fuse || half_tiles) return p;
    const DevLayer &D = c->dm.layer[l];
    const int hd = c->cfg.n_heads;
    const double *acc = stat_acc + (size_t)l * kVnReplicas * 2 * hd;
    p.vn = vn_fuse_args(c, sp, l, x_next, nullptr, 2);
    p.stats_done = true;
    const bool to_ddpm = !has_next && l == c->cfg.num_layers - 1 && out_pos && c->opt.ddpm_fold && chain_guide(c) == Guide::None &&
                         c->cfg.num_classes <= 16 && hd <= 16;
    if (fold && has_next) p.pending = VnFold{c->pd, acc, c->P(D.bn_g), c->P(D.bn_b), c->xsum, cur_x, x_next, c->mol_span, c->status + ST_SPAN, 1};
    else if (fold && to_ddpm) p.ddpm = DdpmFold{c->pd, acc, c->P(D.bn_g), c->P(D.bn_b), c->xsum, cur_x, out_pos, hd, 1};
    else return p;
    p.xsum = c->xsum;
    p.vn_done = true;
    return p;
}

// The per-atom node prologue (node_prologue6_kernel / node_prologue16_kernel of the node precision mode in use): its arguments
// without the per-evaluation bookkeeping, and its launch
template <int H>
NodePrologueArgs prologue_args(const shapemol_ctx *c, const int64_t *v, const int *mol_of, const int *t_mol, const float *add_mol,
                               float *h_out, float *q_out, float *pre_out, int n) {
    const DevLayer &D0 = c->dm.layer[0];
    NodePrologueArgs pa{};
    pa.emb_wT = c->P(c->dm.embwT); pa.emb_b = c->P(c->dm.embb); pa.v = v; pa.mol_of = mol_of; pa.ttab = c->ttab; pa.etab = c->etab; pa.t_mol = t_mol;
    pa.h_out = h_out;
    pa.q = follow_of(c, D0.q_x2h, NODE_LN_RELU, q_out, H, H);
    pa.lin_img6 = c->P(c->opt.node_f16 ? D0.pre16_x2h : D0.pre6_x2h); pa.add_mol = add_mol; pa.pre_out = pre_out;
    pa.n_lin_tiles = 4 * (H / 16); pa.ld_add = 4 * H; pa.ld_out = 4 * H;
    pa.n_atoms = n; pa.C = c->cfg.num_classes; pa.D = c->cfg.time_emb_dim;
    return pa;
}

template <int H>
int launch_prologue(shapemol_ctx *c, hipStream_t s, const NodePrologueArgs &pa, int *range_flag = nullptr) {
    const int n_ct = (pa.n_atoms + 15) / 16;
    const dim3 grid((n_ct + CHAIN_COLS - 1) / CHAIN_COLS), block(H * 4);
    if (!range_flag) range_flag = c->status + ST_RANGE;
    if (c->opt.node_f16 && c->opt.feat_f16) LAUNCH("node_prologue", SMK((node_prologue16_kernel<H, true>), grid, block, Prologue16Lds<H>::BYTES, s, pa, range_flag));
    else if (c->opt.node_f16) LAUNCH("node_prologue", SMK(node_prologue16_kernel<H>, grid, block, Prologue16Lds<H>::BYTES, s, pa, range_flag));
    else LAUNCH("node_prologue", SMK(node_prologue6_kernel<H>, grid, block, Prologue6Lds<H>::BYTES, s, pa));
    return 0;
}

// The node chain in one launch per pair of column tiles, in the form the node precision options select (chain_bf16, node_f16, feat_f16)
template <int H>
int launch_node_chain(shapemol_ctx *c, hipStream_t s, const NodeChainArgs &na) {
    const int n_ct = (na.n_atoms + 15) / 16;
    const dim3 grid((n_ct + CHAIN_COLS - 1) / CHAIN_COLS), block(H * 4);
    if (c->opt.chain_bf16 && c->opt.node_f16 && c->opt.feat_f16) LAUNCH("node_chain", SMK((node_chain16_kernel<H, true>), grid, block, Chain16Lds<H>::BYTES, s, na, c->status + ST_RANGE));
    else if (c->opt.chain_bf16 && c->opt.node_f16) LAUNCH("node_chain", SMK(node_chain16_kernel<H>, grid, block, Chain16Lds<H>::BYTES, s, na, c->status + ST_RANGE));
    else if (c->opt.chain_bf16) LAUNCH("node_chain", SMK(node_chain6_kernel<H>, grid, block, Chain6Lds<H>::BYTES, s, na));
    else LAUNCH("node_chain", SMK(node_chain_kernel<H>, grid, block, 0, s, na));
    return 0;
}

// which of the three prologue kernels the node precision options select; the tables are keyed by it
int prologue_tab_key(const shapemol_ctx *c) { return 1 + (c->opt.node_f16 ? 1 + (c->opt.feat_f16 ? 1 : 0) : 0); }

// q_tab / pre_tab for the precision mode in use, on the stream of the evaluation that needs them (before any graph capture: the
// first build allocates).  Built with the prologue kernel itself over the pseudo-batch of T x C atoms, atom (t, c) of type c at
// timestep t, without a per-molecule term: the table rows are the bits that kernel writes for a real atom with that pair.
// (Its h0 output goes back onto the etab rows it was read from, unchanged.)
template <int H>
int ensure_prologue_tables(shapemol_ctx *c, hipStream_t s) {
    if (!c->opt.prologue_tab || !(c->opt.chain_bf16 && c->opt.lin_bf16) || c->tab_key == prologue_tab_key(c)) return 0;
    const int T = c->cfg.num_timesteps, C = c->cfg.num_classes;
    const size_t rows = (size_t)T * C;
    if (!c->q_tab) {
        HIPCHK(c->mem_tab.alloc(&c->q_tab, rows * 5 * H * sizeof(float) + rows * (sizeof(int64_t) + sizeof(int)) + ((size_t)T + 1) * sizeof(int)));
        c->pre_tab = c->q_tab + rows * H;
        c->tab_v = reinterpret_cast<int64_t *>(c->pre_tab + rows * 4 * H);
        c->tab_mol_of = reinterpret_cast<int *>(c->tab_v + rows); c->tab_t_mol = c->tab_mol_of + rows; c->tab_flag = c->tab_t_mol + T;
    }
    c->tab_key = 0;
    LAUNCH("prep", SMK(prologue_tab_index_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, c->tab_v, c->tab_mol_of, c->tab_t_mol, c->tab_flag, T, C));
    const NodePrologueArgs pa = prologue_args<H>(c, c->tab_v, c->tab_mol_of, c->tab_t_mol, nullptr, c->etab, c->q_tab, c->pre_tab, (int)rows);
    if (launch_prologue<H>(c, s, pa, c->tab_flag)) return 1;
    c->tab_key = prologue_tab_key(c);
    return 0;
}

// One score evaluation on prepared batch data and the prepared shape data sp.  x_in/v_in: current state; outputs as given.
template <int H>
int run_score(shapemol_ctx *c, hipStream_t s, const ShapePrep &sp, const float *x_in, const int64_t *v_in, int64_t N, int64_t B,
              bool sampling, int t_first, float *out_pos, float *out_h, float *out_v, bool reuse_graph = false) {
    // reuse_graph: the second (unconditional) evaluation of a guided step on the same positions keeps the step's kNN graph
    // and edge weights (nbr, ew)
    const shapemol_config &g = c->cfg;
    const int L = g.num_layers, hd = g.n_heads, C = g.num_classes, D = g.time_emb_dim, KP = c->KP;
    const int n = (int)N;
    AtomEmbArgs ae{c->P(c->dm.embw), c->P(c->dm.embb), v_in, c->mol_of, c->ttab, c->t_mol, sampling ? c->steps : nullptr,
                   c->steps + 1, c->bn_acc, c->h_a, n, H, C, D, t_first, L * kVnReplicas * 2 * hd + L};   // + the grid-barrier counters
    const int nlay = c->opt.stop_layer >= 0 ? std::min(c->opt.stop_layer, L) : L;
    // every decision that does not depend on the layer, from the geometry of the launches below (sm_launch.h)
    const lg::In gi = launch_in<H>(c, n);
    const lg::StepForms sf = lg::step_forms(gi, sampling, c->n_pins > 0);
    if (sf.fused_prologue && c->opt.prologue_tab) {      // the same three outputs, gathered from the per-(timestep, type) tables
        if (c->tab_key != prologue_tab_key(c)) return fail("run_score: the prologue tables are not built for this precision mode");
        PrologueTabArgs ta{c->etab, c->q_tab, c->pre_tab, c->tab_flag, v_in, c->mol_of, c->t_mol, ae.step_ptr, ae.step_cur, c->bn_acc,
                           sp.add0, c->h_a, c->q_x, c->pre0, c->status + ST_RANGE, n, C, g.num_timesteps, t_first, ae.bn_acc_len};
        LAUNCH("node_prologue", SMK(node_prologue_tab_kernel<H>, dim3((unsigned)((N * 16 + kProTabThreads - 1) / kProTabThreads)), dim3(kProTabThreads), 0, s, ta));
    } else if (sf.fused_prologue) {
        NodePrologueArgs pa = prologue_args<H>(c, v_in, c->mol_of, c->t_mol, sp.add0, c->h_a, c->q_x, c->pre0, n);
        pa.step_ptr = ae.step_ptr; pa.step_cur = ae.step_cur; pa.bn_acc = c->bn_acc; pa.bn_acc_len = ae.bn_acc_len; pa.t_first = t_first;
        if (nlay == 0) pa.n_lin_tiles = 0;
        pa.stamps = c->kstamp_sel == 5 ? c->kstamps : nullptr;
        if (launch_prologue<H>(c, s, pa)) return 1;
    } else {
        LAUNCH("embed", SMK(atom_embed_kernel, dim3((N * H + 255) / 256), dim3(256), 0, s, ae));
    }
    int64_t (&rec)[8] = c->launch_rec;
    std::fill(rec, rec + 8, 0);
    std::fill(c->node_rec, c->node_rec + 8, 0);
    std::fill(c->x2h_out_rec, c->x2h_out_rec + 4, 0);
    rec[0] = sampling; rec[1] = sf.graph_fused; rec[7] = c->num_cu;
    { const int64_t er[4] = {sf.half_tiles, lg::tile_jobs(KP, n).jobs, 0, sf.half_tiles ? H : 0}; std::copy(er, er + 4, c->edge_rec); }
    if (sf.stream && nlay > 0) { const lg::StreamGeom g = lg::stream_geom(gi); rec[5] = g.chunk; rec[6] = g.grid; }
    if (reuse_graph) {
    } else if (sf.graph_fused) {
        GraphArgs ga{x_in, c->mol_span, n, g.knn, KP, c->nbr, c->P(c->dm.ew.w1), c->P(c->dm.ew.b1), c->P(c->dm.ew.g), c->P(c->dm.ew.be),
                     c->P(c->dm.ew.w2), c->P(c->dm.ew.b2), c->ew, c->status + ST_SPAN, c->kstamp_sel == 4 ? c->kstamps : nullptr};
        const int apb = kGraphWaves * (KP >= 16 ? 1 : 16 / KP);      // atoms per workgroup
        DISPATCH_KP("graph", graph_kernel, (), dim3((n + apb - 1) / apb), dim3(kGraphWaves * 64), 0, s, ga);
    } else LAUNCH("knn", SMK(knn_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x_in, c->mol_of, c->mol_off, n, g.knn, KP, c->nbr));
    if (sampling && c->n_pins > 0 && !reuse_graph)      // diagnostic: the pinned atoms of this reverse step take the given neighbour lists
        LAUNCH("knn", SMK(knn_pin_kernel, dim3(32), dim3(256), 0, s, c->pin_off, c->pin_steps, c->pin_atom, c->pin_nbr, c->pin_k, KP, c->steps + 1, n, c->nbr));
    EdgeWeightArgs ea{x_in, c->nbr, c->P(c->dm.ew.w1), c->P(c->dm.ew.b1), c->P(c->dm.ew.g), c->P(c->dm.ew.be),
                      c->P(c->dm.ew.w2), c->P(c->dm.ew.b2), c->ew, n * KP, KP};
    if (!sf.graph_fused && !reuse_graph) {
        const int tiles = (n * KP + 15) / 16;
        LAUNCH("edge_weight", SMK(edge_weight_kernel<H>, dim3((tiles + 3) / 4), dim3(256), 0, s, ea));
    }
    const float *cur_x = x_in;
    float *cur_h = c->h_a;
    constexpr int NT = H / 16;
    bool v_done = false;
    if (nlay > 0 && !sf.fused_prologue) {   // prologue: per-node products and queries of the first x2h attention
        const DevLayer &D0 = c->dm.layer[0];
        if (launch_linear<H>(c, s, "node_pre", cur_h, c->P(D0.pre_x2h), c->P(D0.pre6_x2h), c->P(D0.pre16_x2h), sp.add0, 4 * H, c->pre0, 4 * H, 4 * NT, n,
                             c->kstamp_sel == 0 ? c->kstamps : nullptr)) return 1;
        if (launch_mlp2<H, 1>(c, s, "node_q", D0.q_x2h, cur_h, nullptr, NODE_LN_RELU, nullptr, c->q_x, H, H, n)) return 1;
    }
    // evaluation-mode batch-norm: the consumers of the batch sums read sums that reproduce the running statistics
    double *stat_acc = c->bn_acc;
    if (c->bn_eval) {
        if (!c->bn_run) return fail("bn_eval = 1 needs the running statistics (shapemol_set_bn_running)");
        if (c->opt.vn_fuse == 1) return fail("bn_eval = 1 is not available with vn_fuse = 1 (coordinate update behind a grid barrier)");
        const int tot = L * kVnReplicas * 2 * hd;
        LAUNCH("prep", SMK(bn_eval_fill_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, c->bn_run, c->bn_run + (size_t)L * hd, L, hd, n, c->bn_eval_acc));
        stat_acc = c->bn_eval_acc;
    }
    VnFold pending{};                         // fold: the x2h kernel of layer l + 1 receives the coordinate update of layer l
    for (int l = 0; l < nlay; ++l) {
        const DevLayer &Dl = c->dm.layer[l];
        const bool last = (l == nlay - 1), has_next = !last;
        const float *pre_x = l == 0 ? c->pre0 : c->preAB + 4 * H;      // node pre-products of this x2h attention
        const int ld_pre_x = l == 0 ? 4 * H : 8 * H;
        unsigned long long *stamps_x = (c->kstamp_sel == 1 && l == 0) ? c->kstamps : nullptr;
        float *h_dst = (last && out_h) ? out_h : (cur_h == c->h_a ? c->h_b : c->h_a);      // h' of this layer
        Edge16Args xea{};
        if (sf.f16 || sf.stream) {   // x2h attention: two-piece f16 operands, both MLP images resident (sm_edge16.h), or exactly split bf16
                               // operands, producer / consumer waves (sm_edge_stream.h); `pending`: the previous layer's coordinate update
            if (sf.f16) {
                xea.image_k = c->P(Dl.i16_kx); xea.image_v = c->P(Dl.i16_vx);
                fill_edge(xea, c, pre_x, ld_pre_x, c->q_x, cur_x, c->att, n, sf.half_tiles, stamps_x);
                xea.vf = pending;
                if (!sf.xc_fused && launch_edge16<H, false>(c, s, xea)) return 1;     // (fused: launched with the node stage below)
            } else {
                EdgeStreamArgs sa{};
                sa.part_k = c->P(Dl.st_kx); sa.part_v = c->P(Dl.st_vx);
                sa.w2k = reinterpret_cast<const unsigned *>(c->P(Dl.sw2_kx)); sa.w2v = reinterpret_cast<const unsigned *>(c->P(Dl.sw2_vx));
                sa.b2v = c->P(Dl.sb2_vx);
                fill_edge(sa, c, pre_x, ld_pre_x, c->q_x, cur_x, c->att, n, sf.half_tiles, stamps_x);
                sa.vf = pending;
                if (sf.out_fused) sa.no = NodeOutArgs{c->att, cur_h, c->P(Dl.no.b1), c->P(Dl.no.g), c->P(Dl.no.be), c->P(Dl.no.b2),
                                                   c->P(Dl.no.w1img6), c->P(Dl.no.w2img6), h_dst};
                if (launch_stream<H, false>(c, s, sa)) return 1;
            }
            pending = VnFold{};
            if (sf.half_tiles && launch_combine32<false>(c, s, c->att, n)) return 1;
        } else if (sf.phases && c->opt.edge_bf16 == 1) {   // x2h attention, key and value phase in one launch
            EdgeFusedArgs fa{c->P(Dl.img_kx), c->P(Dl.img_vx), pre_x, c->q_x, cur_x, c->nbr, c->ew, c->alpha, c->att, n, ld_pre_x, stamps_x};
            if (launch_fused<H, false>(c, s, fa)) return 1;
        } else {   // x2h attention (fp32 MFMA kernels)
            EdgeArgs e{c->P(Dl.blob_x2h), pre_x, c->q_x, cur_x, c->nbr, c->ew, c->att, n, ld_pre_x, stamps_x};
            if (launch_edge<H, false>(c, s, e)) return 1;
        }
        {   // node side: h' = h + MLP([att | h]); queries of h2x (this layer) and x2h (next layer) or the v head
            float *dst = h_dst;
            NodeChainArgs na{};
            na.att = c->att; na.h = cur_h; na.h_out = dst; na.n_atoms = n;
            na.stamps = (c->kstamp_sel == 3 && l == 0) ? c->kstamps : nullptr;
            na.w1img = c->P(Dl.no.w1img); na.b1 = c->P(Dl.no.b1); na.ln_g = c->P(Dl.no.g); na.ln_b = c->P(Dl.no.be);
            na.w2img = c->P(Dl.no.w2img); na.b2 = c->P(Dl.no.b2);
            na.w1img6 = c->P(c->opt.node_f16 ? Dl.no.w1img16 : Dl.no.w1img6); na.w2img6 = c->P(c->opt.node_f16 ? Dl.no.w2img16 : Dl.no.w2img6);
            na.f[0] = follow_of(c, Dl.q_h2x, NODE_LN_RELU, c->q_h, H, H);
            na.n_follow = 1;
            if (has_next) { na.f[1] = follow_of(c, c->dm.layer[l + 1].q_x2h, NODE_LN_RELU, c->q_x, H, H); na.n_follow = 2; }
            else if (out_v) { na.f[1] = follow_of(c, c->dm.vhead, NODE_SSP, out_v, C, C); na.n_follow = 2; v_done = true; }
            const int lin_tiles = (has_next && l + 1 < L ? 8 : 4) * NT;
            if (sf.lin_fused) {
                na.lin_img16 = c->P(Dl.lin16_img); na.add_mol = sp.addp + (size_t)l * c->capB * 8 * H; na.mol_of = c->mol_of;
                na.pre_out = c->preAB; na.n_lin_tiles = lin_tiles; na.ld_add = 8 * H; na.ld_out = 8 * H;
            }
            float *lin_add = sp.addp + (size_t)l * c->capB * 8 * H;
            if (sf.levels) { if (launch_node_levels<H>(c, s, na, c->P(Dl.lin6_img), lin_add, 8 * H, c->preAB, 8 * H, lin_tiles, sf.out_fused)) return 1; }
            else if (sf.xc_fused) { rec[4] = 1; if (launch_x2h_chain<H>(c, s, xea, na)) return 1; }
            else if (launch_node_chain<H>(c, s, na)) return 1;
            cur_h = dst;
            // per-node halves of the edge MLPs' first Linear: h2x of this layer | x2h of the next one
            if (!sf.lin_fused && !sf.levels && launch_linear<H>(c, s, "node_pre", cur_h, c->P(Dl.lin_img), c->P(Dl.lin6_img), c->P(Dl.lin16_img), lin_add, 8 * H,
                                 c->preAB, 8 * H, lin_tiles, n, (c->kstamp_sel == 0 && l == 0) ? c->kstamps : nullptr)) return 1;
        }
        float *x_next = (last && out_pos) ? out_pos : ((cur_x == c->x_a) ? c->x_b : c->x_a);
        bool vn_done = false, stats_done = false;
        unsigned long long *stamps_h = (c->kstamp_sel == 2 && l == 0) ? c->kstamps : nullptr;
        if ((sf.f16 || sf.stream) && c->opt.vn_fuse != 1) {   // h2x attention (+ VN-linear and batch statistics when vn_fuse = 2)
            const H2xPlan plan = h2x_plan(c, sp, l, sf.fold, has_next, sf.half_tiles, stat_acc, cur_x, x_next, out_pos);
            pending = plan.pending; stats_done = plan.stats_done; vn_done = plan.vn_done;
            if (plan.ddpm.enable) c->ddpm_vf = plan.ddpm;
            rec[2] |= plan.pending.enable; rec[3] |= plan.ddpm.enable;
            if (sf.f16) {
                Edge16Args ea{};
                ea.image_k = c->P(Dl.i16_kh); ea.image_v = c->P(Dl.i16_vh);
                fill_edge(ea, c, c->preAB, 8 * H, c->q_h, cur_x, c->o3, n, sf.half_tiles, stamps_h);
                ea.vn = plan.vn; ea.xsum = plan.xsum;
                if (launch_edge16<H, true>(c, s, ea)) return 1;
            } else {
                EdgeStreamArgs sa{};
                sa.part_k = c->P(Dl.st_kh); sa.part_v = c->P(Dl.st_vh);
                sa.w2k = reinterpret_cast<const unsigned *>(c->P(Dl.sw2_kh));
                fill_edge(sa, c, c->preAB, 8 * H, c->q_h, cur_x, c->o3, n, sf.half_tiles, stamps_h);
                sa.vn = plan.vn; sa.xsum = plan.xsum;
                if (launch_stream<H, true>(c, s, sa)) return 1;
            }
            if (sf.half_tiles && launch_combine32<true>(c, s, c->o3, n)) return 1;
        } else if (sf.phases) {   // h2x attention, both images resident in LDS (exactly split bf16 operands)
            EdgeFusedArgs fa{c->P(Dl.img_kh), c->P(Dl.img_vh), c->preAB, c->q_h, cur_x, c->nbr, c->ew, c->alpha, c->o3, n, 8 * H, stamps_h};
            if (c->opt.vn_fuse) {   // VN-linear + batch statistics (2) or the whole coordinate update (1: grid barrier inside) behind the attention
                double *tail = c->bn_acc + (size_t)L * kVnReplicas * 2 * hd;
                fa.vn = vn_fuse_args(c, sp, l, x_next, reinterpret_cast<unsigned *>(tail + l), c->opt.vn_fuse == 1 ? 1 : 2);
                if (c->opt.vn_fuse == 1) vn_done = true; else stats_done = true;
            }
            if (launch_fused<H, true>(c, s, fa)) return 1;
        } else {   // h2x attention (fp32 MFMA kernels)
            EdgeArgs e{c->P(Dl.blob_h2x), c->preAB, c->q_h, cur_x, c->nbr, c->ew, c->o3, n, 8 * H, stamps_h};
            if (launch_edge<H, true>(c, s, e)) return 1;
        }
        VnArgs va{cur_x, c->o3, sp.ps + (size_t)l * c->capB * 2 * hd * 3, c->P(Dl.wf_x), c->P(Dl.wd_x), c->P(Dl.wf_o),
                  c->P(Dl.wd_o), c->P(Dl.bn_g), c->P(Dl.bn_b), c->mol_of, c->pd, c->bn_acc + (size_t)l * kVnReplicas * 2 * hd, x_next, n, hd};
        const int per_blk = 256 / hd;
        if (!vn_done) {
            if (!stats_done) LAUNCH("vn_stats", SMK(vn_stats_kernel, dim3((N + per_blk - 1) / per_blk), dim3(kVnThreads), 0, s, va));
            if (c->bn_eval) va.acc = stat_acc + (size_t)l * kVnReplicas * 2 * hd;      // (the statistics pass wrote the batch's sums elsewhere)
            LAUNCH("vn_apply", SMK(vn_apply_kernel, dim3((N + per_blk - 1) / per_blk), dim3(256), 0, s, va));
        }
        cur_x = x_next;
    }
    c->last_h = cur_h; c->last_x = cur_x;
    if (nlay == 0 && out_pos) HIPCHK(hipMemcpyAsync(out_pos, x_in, N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out_v && !v_done) {
        if (launch_mlp2<H, 1>(c, s, "v_head", c->dm.vhead, cur_h, nullptr, NODE_SSP, nullptr, out_v, C, C, n)) return 1;
    }
    return 0;
}

template <int H>
int run_ddpm(shapemol_ctx *c, hipStream_t s, int64_t N) {
    const shapemol_config &g = c->cfg;
    DdpmArgs a{};
    a.pred_pos = c->pred_pos; a.pred_v = c->pred_v; a.x_t = c->x_state; a.v_t = c->v_state; a.mol_of = c->mol_of;
    a.t_first = c->cfg.num_timesteps - 1;
    a.c0 = c->P(c->dm.tab[0]); a.ct = c->P(c->dm.tab[1]); a.logvar = c->P(c->dm.tab[2]); a.log_a = c->P(c->dm.tab[3]);
    a.log_1ma = c->P(c->dm.tab[4]); a.log_abar = c->P(c->dm.tab[5]); a.log_1mabar = c->P(c->dm.tab[6]);
    a.cp = c->chain_params; a.step_cur = c->steps + 1; a.step_ptr = c->steps;
    a.x_next = c->x_state; a.v_next = c->v_state;
    a.n_atoms = (int)N; a.C = g.num_classes;
    a.vf = c->ddpm_vf; c->ddpm_vf = DdpmFold{};
    const CfgArgs cfg = cfg_args(c, N);
    if (c->stamp_on) LAUNCH("stamp", SMK(clock_stamp_kernel, dim3(1), dim3(64), 0, s, c->stamps, c->steps + 1, 1024));
    if (g.num_classes <= 16) LAUNCH("ddpm", SMK(ddpm_step16_kernel, dim3((N * 16 + 255) / 256), dim3(256), 0, s, a, cfg));
    else LAUNCH("ddpm", SMK(ddpm_step_kernel<32>, dim3((N + 127) / 128), dim3(128), 0, s, a, cfg));
    return 0;
}

int check_cfg(const shapemol_config &g) {
    if (g.hidden_dim != 128 && g.hidden_dim != 32) return fail("hidden_dim must be 128 (or 32 for the reduced test model)");
    if (g.n_heads * 8 != g.hidden_dim) return fail("hidden_dim / n_heads must be 8");
    if (g.num_r_gaussian != 20) return fail("num_r_gaussian must be 20 (fixed RBF centres)");
    if (g.knn < 1 || g.knn > 32) return fail("knn must be in 1..32");
    // k > 16 runs on half-atom tiles, whose h2x rows are 48 floats wide and are stored into rows of hidden_dim floats (part_rows):
    // at hidden_dim 32 they do not fit, and a forward of that combination has faulted on the device
    if (g.knn > 16 && g.hidden_dim < 48) return fail("knn > 16 needs hidden_dim 128 (the reduced model, hidden_dim 32, supports knn 1..16)");
    if (g.shape_dim < 1 || g.shape_dim > 64 || g.shape_latent_dim < 4 || g.shape_latent_dim > 64 || (g.shape_latent_dim & 3))
        return fail("shape_dim must be 1..64, shape_latent_dim a multiple of 4 in 4..64");
    if (g.time_emb_dim < 4 || g.time_emb_dim > 16 || (g.time_emb_dim & 1)) return fail("time_emb_dim must be even, 4..16");
    if (g.num_classes < 2 || g.num_classes > 32) return fail("num_classes must be 2..32");
    if (g.num_layers < 1 || g.num_timesteps < 1) return fail("num_layers / num_timesteps must be positive");
    return 0;
}

// f(std::integral_constant<int, H>) for the context's hidden width: f is a generic lambda that names a template as f<h()>
template <typename F>
auto dispatch_h(const shapemol_ctx *c, F &&f) {
    return c->cfg.hidden_dim == 128 ? f(std::integral_constant<int, 128>{}) : f(std::integral_constant<int, 32>{});
}

}  // namespace

// =================================================================================================
extern "C" {

int shapemol_abi_version(void) { return SHAPEMOL_ABI_VERSION; }
void shapemol_set_error_(const char *msg) { g_err = msg ? msg : ""; }      // other translation units of the library
const char *shapemol_last_error(void) { return g_err.c_str(); }

size_t shapemol_weight_count(const shapemol_config *cfg) { return cfg ? weight_count(*cfg) : 0; }

int shapemol_create(const shapemol_config *cfg, const float *weights, size_t n_weights, int device, shapemol_ctx **out) {
    if (!cfg || !weights || !out) return fail("shapemol_create: null argument");
    if (check_cfg(*cfg)) return 1;
    if (n_weights != weight_count(*cfg)) return fail("shapemol_create: weight count mismatch (got " + std::to_string(n_weights) + ", want " + std::to_string(weight_count(*cfg)) + ")");
    HostModel hm;
    if (!parse_weights(*cfg, weights, n_weights, hm)) return fail("shapemol_create: weight layout mismatch");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("shapemol_create: no such HIP device");
    HIPCHK(hipSetDevice(device));
    auto *c = new shapemol_ctx();
    auto drop = [&](int rc) { shapemol_destroy(c); return rc; };     // every pointer starts null: a partly built context is destroyed like a whole one
    c->cfg = *cfg; c->device = device;
    c->KP = cfg->knn <= 8 ? 8 : (cfg->knn <= 16 ? 16 : 32);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return drop(hip_fail("hipGetDeviceProperties", e));
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    Image im;
    if (build_model_image(*cfg, hm, im, c->dm, c->hid_max)) return drop(1);
    const DevModel &dm = c->dm;
    const int H = cfg->hidden_dim, T = cfg->num_timesteps, C = cfg->num_classes;
    if ((e = c->mem_model.alloc(&c->d_img, im.d.size() * sizeof(float))) != hipSuccess) return drop(hip_fail("shapemol_create: weights", e));
    if ((e = hipMemcpy(c->d_img, im.d.data(), im.d.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return drop(hip_fail("hipMemcpy(weights)", e));
    if (dispatch_h(c, [&](auto h) { return set_edge_attr<h()>(c->KP); })) return drop(1);
    // time-embedding table over all timesteps, and the atom embedding of every (timestep, atom type) pair
    if ((e = c->mem_model.alloc(&c->ttab, (size_t)T * cfg->time_emb_dim * sizeof(float))) != hipSuccess) return drop(hip_fail("shapemol_create: time table", e));
    if ((e = c->mem_model.alloc(&c->etab, (size_t)T * C * H * sizeof(float))) != hipSuccess) return drop(hip_fail("shapemol_create: embedding table", e));
    TimeTableArgs ta{c->P(dm.te1w), c->P(dm.te1b), c->P(dm.te2w), c->P(dm.te2b), c->ttab, T, cfg->time_emb_dim};
    hipLaunchKernelGGL(time_table_kernel, dim3((T + 63) / 64), dim3(64), 0, nullptr, ta);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return drop(hip_fail("time table kernel", e));
    const int items = T * C * (H / 4);
    hipLaunchKernelGGL(emb_table_kernel, dim3((items + 255) / 256), dim3(256), 0, nullptr, c->P(dm.embwT), c->P(dm.embb), c->ttab, c->etab, T, C, cfg->time_emb_dim, H);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return drop(hip_fail("embedding table kernel", e));
    // (the default kernels split every operand into bf16 pieces, which have the fp32 exponent range: no bound on the weights.  The
    //  optional two-piece f16 kernels, edge_bf16 = 3, refuse weights whose LayerNorm outputs could leave the fp16 range: hid_max)
    *out = c;
    return 0;
}

void shapemol_destroy(shapemol_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    c->drop_graphs();
    for (auto &r : c->prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    delete c;                 // its lists release what they own
}

int shapemol_set_bn_running(shapemol_ctx *c, const float *h_mean, const float *h_var, int64_t count) {
    if (!c || !h_mean || !h_var) return fail("shapemol_set_bn_running: null argument");
    const int L = c->cfg.num_layers, hd = c->cfg.n_heads;
    if (count != (int64_t)L * hd) return fail("shapemol_set_bn_running: count must be num_layers * n_heads");
    for (int64_t i = 0; i < count; ++i)
        if (!(h_var[i] >= 0.f) || !std::isfinite(h_mean[i]) || !std::isfinite(h_var[i])) return fail("shapemol_set_bn_running: statistics must be finite, variance >= 0");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (!c->bn_run) {      // (a failed second allocation releases the first: both or neither)
        HIPCHK(c->mem_bn.alloc(&c->bn_run, 2 * count * sizeof(float)));
        HIPCHK(c->mem_bn.alloc(&c->bn_eval_acc, (size_t)L * kVnReplicas * 2 * hd * sizeof(double)));
    }
    HIPCHK(hipMemcpy(c->bn_run, h_mean, count * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->bn_run + count, h_var, count * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int shapemol_reserve(shapemol_ctx *c, int64_t max_atoms, int64_t max_mols) {
    if (!c || max_atoms < 1 || max_mols < 1) return fail("shapemol_reserve: bad argument");
    return ensure_workspace(c, max_atoms, max_mols);
}

int shapemol_score(shapemol_ctx *c, const float *d_pos, const int64_t *d_v, const int64_t *d_batch, int64_t N,
                   int64_t B, const float *d_shape, const int64_t *d_t, float *out_pos, float *out_h, float *out_v,
                   void *stream) {
    if (!c || !d_pos || !d_v || !d_batch || !d_shape || !d_t || !out_pos || !out_v) return fail("shapemol_score: null argument");
    if (N < 1 || B < 1 || N > (1 << 27)) return fail("shapemol_score: n_atoms / n_mols out of range");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, B)) return 1;
    hipStream_t s = (hipStream_t)stream;
    c->lastN = N; c->lastB = B;
    if (dispatch_h(c, [&](auto h) { return ensure_prologue_tables<h()>(c, s); })) return 1;
    HIPCHK(hipMemsetAsync(c->status, 0, 8 * sizeof(int), s));
    if (dispatch_h(c, [&](auto h) { return run_prep<h()>(c, s, d_batch, N, B, d_shape, c->prep[0]); })) return 1;
    LAUNCH("prep", SMK(t_convert_kernel, dim3((B + 255) / 256), dim3(256), 0, s, d_t, (int)B, c->cfg.num_timesteps, c->t_mol, c->status));
    LAUNCH("prep", SMK(v_check_kernel, dim3((N + 255) / 256), dim3(256), 0, s, d_v, (int)N, c->cfg.num_classes, c->status));
    return dispatch_h(c, [&](auto h) { return run_score<h()>(c, s, c->prep[0], d_pos, d_v, N, B, false, 0, out_pos, out_h, out_v); });
}

int shapemol_sample(shapemol_ctx *c, const float *d_init_pos, const int64_t *d_init_v, const int64_t *d_batch,
                    int64_t N, int64_t B, const float *d_shape, int32_t num_steps, const float *d_eps, const float *d_u,
                    uint64_t seed, const shapemol_traj *traj, float *out_pos, int64_t *out_v, int32_t use_graph, void *stream) {
    if (!c || !d_init_pos || !d_init_v || !d_batch || !d_shape || !out_pos || !out_v) return fail("shapemol_sample: null argument");
    if (N < 1 || B < 1 || N > (1 << 27)) return fail("shapemol_sample: n_atoms / n_mols out of range");
    if (num_steps < 1 || c->first_step + num_steps > c->cfg.num_timesteps) return fail("shapemol_sample: num_steps out of range");
    if ((d_eps == nullptr) != (d_u == nullptr)) return fail("shapemol_sample: d_eps and d_u must be given together");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, B)) return 1;
    hipStream_t s = (hipStream_t)stream;
    c->lastN = N; c->lastB = B;
    if (dispatch_h(c, [&](auto h) { return ensure_prologue_tables<h()>(c, s); })) return 1;
    const int t_first = c->cfg.num_timesteps - 1;
    const Guide kind = chain_guide(c);
    const bool mesh = kind == Guide::Mesh, cfg = kind == Guide::Cfg;
    if (mesh && mesh_workspace(c, N, c->ms.groups)) return 1;
    if (c->ms.groups > 0 && !c->ms.whole && c->ms.mols != B)        // (groups that are set must fit the batch even where another kind, or none, guides)
        return fail("shapemol_sample: n_mols = " + std::to_string(B) + " but the mesh guidance groups cover " + std::to_string(c->ms.mols) + " molecules");
    if (c->cs.groups > 0 && !c->cs.whole && c->cs.mols != B)
        return fail("shapemol_sample: n_mols = " + std::to_string(B) + " but the guidance groups cover " + std::to_string(c->cs.mols) + " molecules");
    if (c->cgs.groups > 0 && c->cgs.mols != B)
        return fail("shapemol_sample: n_mols = " + std::to_string(B) + " but the classifier-free guidance groups cover " + std::to_string(c->cgs.mols) + " molecules");
    if (kind == Guide::Cloud && groups_table(c, s, c->cs.whole ? nullptr : d_batch, N, c->cs.ints, c->cs.groups)) return 1;
    if (mesh && groups_table(c, s, c->ms.whole ? nullptr : d_batch, N, c->ms.ints, c->ms.groups)) return 1;
    HIPCHK(hipMemsetAsync(c->status, 0, 8 * sizeof(int), s));
    if (mesh && mesh_counters_clear(c, s, c->ms.groups)) return 1;
    if (dispatch_h(c, [&](auto h) { return run_prep<h()>(c, s, d_batch, N, B, d_shape, c->prep[0]); })) return 1;
    uint64_t field_gen = 0;
    if (kind == Guide::Field) {      // the decoder's per-shape prologue of the chain's own shapes, once per chain
        if (shapemol_sd_chain_prepare_(c->field_sd, d_shape, B, s, &field_gen)) return 1;      // (not a profiled launch: no event pair)
    }
    if (cfg) {      // classifier-free guidance: the unconditional evaluation's shape data, from a zeroed shape, once per chain
        if (dispatch_h(c, [&](auto h) { return run_prep_shape<h()>(c, s, B, c->shape_zero, c->prep[1]); })) return 1;
        if (run_cfg_prep(c, s, d_batch, N, B)) return 1;
    }
    LAUNCH("prep", SMK(v_check_kernel, dim3((N + 255) / 256), dim3(256), 0, s, d_init_v, (int)N, c->cfg.num_classes, c->status));
    {
        ChainParams cp{};
        cp.seed = seed; cp.eps = d_eps; cp.u = d_u; cp.step_base = c->first_step; cp.guide_draws = mesh ? c->ms.draws : c->cs.draws;
        if (traj) { cp.tr_pos = traj->pos_traj; cp.tr_v = traj->v_traj; cp.tr_v0 = traj->v0_traj; cp.tr_vt = traj->vt_traj;
                    cp.tr_pos_cond = traj->pos_cond_traj; cp.tr_v_cond = traj->v_cond_traj; }
        if (cfg && c->cgs.groups > 0) { cp.tr_pos_uncond = c->cgs.tr_pos_u; cp.tr_v_uncond = c->cgs.tr_v_u; }
        else if (cfg) { cp.tr_pos_uncond = c->cfg_tr_pos_u; cp.tr_v_uncond = c->cfg_tr_v_u; }
        LAUNCH("prep", SMK(set_chain_params_kernel, dim3(1), dim3(1), 0, s, c->chain_params, cp, c->steps));
    }
    HIPCHK(hipMemcpyAsync(c->x_state, d_init_pos, N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->v_state, d_init_v, N * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    auto one_step = [&]() -> int {
        if (dispatch_h(c, [&](auto h) { return run_score<h()>(c, s, c->prep[0], c->x_state, c->v_state, N, B, true, t_first, c->pred_pos, nullptr, c->pred_v); })) return 1;
        if (cfg) {        // the same step on a zeroed shape: same positions, graph and step index; own batch statistics and outputs
            if (dispatch_h(c, [&](auto h) { return run_score<h()>(c, s, c->prep[1], c->x_state, c->v_state, N, B, true, t_first, c->pred_pos_u, nullptr, c->pred_v_u, true); }) ||
                run_cfg_stats(c, s, cfg_args(c, N))) return 1;
        }
        if (enqueue_guidance(c, s, kind, c->pred_pos, N, c->steps + 1, t_first)) return 1;     // shape guidance of the predicted x0 (steps with t > grad_step)
        return dispatch_h(c, [&](auto h) { return run_ddpm<h()>(c, s, N); });
    };
    if (use_graph && !c->prof_on) {
        shapemol_ctx::GraphKey key{};
        // (the forms run_score will choose: same call, same arguments)
        const lg::StepForms sf = dispatch_h(c, [&](auto h) { return lg::step_forms(launch_in<h()>(c, (int)N), true, c->n_pins > 0); });
        key.N = N; key.B = B; key.guide = kind; key.fold = sf.fold; key.gfuse = sf.graph_fused;
        if (kind == Guide::Field) { key.field_gen = field_gen; key.field_lr = c->field_lr; key.field_step = c->field_step; }
        if (cfg && c->cgs.groups > 0) {
            key.cfg = 1 + c->cgs.type; key.cfg_groups = c->cgs.groups; key.cfgv[1] = c->cgs.p;
        } else if (cfg) {
            key.cfg = 1 + c->cfg_type;
            const double v[9] = {c->cfg_w, c->cfg_p, (double)c->cfg_has_bounds, c->cfg_lo[0], c->cfg_lo[1], c->cfg_lo[2], c->cfg_hi[0], c->cfg_hi[1], c->cfg_hi[2]};
            std::copy(v, v + 9, key.cfgv);
        }
        // two executables: one reverse step, and kGraphUnroll steps back to back (the gap between two graph launches,
        // ~8 us, is then paid once per kGraphUnroll steps); every step reads its index from the device-side counter
        auto capture = [&](int n_steps, hipGraphExec_t *exec) -> int {
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            int rc = 0;
            for (int i = 0; i < n_steps && !rc; ++i) rc = one_step();
            const hipError_t ce = hipStreamEndCapture(s, &graph);
            if (rc) { if (graph) hipGraphDestroy(graph); return 1; }
            if (ce != hipSuccess) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            const hipError_t ie = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
            hipGraphDestroy(graph);
            if (ie != hipSuccess) { *exec = nullptr; return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ie)); }
            ++c->n_captures;
            hipGraphUpload(*exec, s);      // stage the executable on the device now, not at its first launch inside a timed chain
            return 0;
        };
        if (!c->gexec || !(key == c->gkey)) {
            c->drop_graphs();
            if (capture(1, &c->gexec)) return 1;
            c->gkey = key;
            std::copy(c->launch_rec, c->launch_rec + 8, c->graph_rec);
        }
        // both executables are built at the first capture, whatever this chain's length: a short warm-up chain then leaves
        // nothing to capture inside a later, timed chain
        if (!c->gexec_u && capture(kGraphUnroll, &c->gexec_u)) return 1;
        int st = 0;
        c->gstream = s; c->gstream_set = true;
        std::copy(c->graph_rec, c->graph_rec + 8, c->launch_rec);      // a replay takes the decisions of its capture
        for (; st + kGraphUnroll <= num_steps; st += kGraphUnroll) HIPCHK(hipGraphLaunch(c->gexec_u, s));
        for (; st < num_steps; ++st) HIPCHK(hipGraphLaunch(c->gexec, s));
    } else {
        for (int st = 0; st < num_steps; ++st) if (one_step()) return 1;
    }
    HIPCHK(hipMemcpyAsync(out_pos, c->x_state, N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out_v, c->v_state, N * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

int shapemol_log_sample_categorical(shapemol_ctx *c, const float *d_logits, const float *d_u, int64_t n_rows,
                                    int32_t n_classes, uint64_t seed, int64_t *out_index, void *stream) {
    if (!d_logits || !out_index || n_rows < 1 || n_classes < 1) return fail("shapemol_log_sample_categorical: bad argument");
    if (c) HIPCHK(hipSetDevice(c->device));      // ctx may be NULL: the current device is used
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gumbel_argmax_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, d_logits, d_u, (int)n_rows, (int)n_classes, seed, out_index);
    HIPCHK(hipGetLastError());
    return 0;
}

int shapemol_set_option(shapemol_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return fail("shapemol_set_option: null argument");
    const std::string k(name);
    if (k == "max_mol_atoms") {   // hint for the folded coordinate update; the captured graph is keyed on the resulting decision
        if (value < 0) return fail("max_mol_atoms must be >= 0");
        c->opt.max_mol_atoms = (int)std::min<int64_t>(value, 1 << 20);
        return 0;
    }
    if (k == "first_step") {      // does not touch the captured graph: the step counter lives in device memory
        if (value < 0 || value >= c->cfg.num_timesteps) return fail("first_step must be in [0, num_timesteps)");
        c->first_step = (int)value;
        return 0;
    }
    if (k == "stop_layer") c->opt.stop_layer = (int)value;
    else if (k == "edge_bf16") {
        if (value < 0 || value > 3) return fail("edge_bf16 must be 0 (fp32 MFMA), 1 (exactly split bf16, phase kernels), 2 (exactly split bf16, streaming kernels) or 3 (two-piece f16)");
        if (value != 3 && value != 2 && c->KP > 16) return fail("k > 16 runs on the streaming (edge_bf16 = 2) or the two-piece f16 (edge_bf16 = 3) edge kernels");
        if (value == 3 && c->hid_max > 6.0e4f) return fail("edge_bf16 = 3: the edge MLPs' LayerNorm outputs may exceed the fp16 range for these weights");
        c->opt.edge_bf16 = (int)value;
    }
    else if (k == "edge_tiles") { if (value < -1 || value > 1) return fail("edge_tiles must be -1 (automatic), 0 (sliced one-job launches) or 1 (looping launch)"); c->opt.edge_tiles = (int)value; }
    else if (k == "node_f16") c->opt.node_f16 = value != 0;
    else if (k == "feat_f16") {
        if (value && (c->opt.edge_bf16 != 3 || !c->opt.node_f16)) return fail("feat_f16 = 1 needs the f16 kernels (edge_bf16 = 3, node_f16 = 1)");
        c->opt.feat_f16 = value != 0;
    }
    else if (k == "lin_fuse") c->opt.lin_fuse = value != 0;
    else if (k == "stream_whole_rounds") c->opt.stream_whole_rounds = value != 0;
    else if (k == "x2h_chain") c->opt.x2h_chain = value != 0;
    else if (k == "graph_fuse") c->opt.graph_fuse = value != 0;
    else if (k == "bn_eval") c->bn_eval = value != 0;
    else if (k == "ddpm_fold") c->opt.ddpm_fold = value != 0;
    else if (k == "vn_fold") c->opt.vn_fold = value != 0;
    else if (k == "prologue_tab") c->opt.prologue_tab = value != 0;      // 0: the per-atom MLP prologue (A/B, equivalence tests)
    else if (k == "lin_bf16") c->opt.lin_bf16 = (int)value;
    else if (k == "chain_bf16") c->opt.chain_bf16 = (int)value;
    else if (k == "vn_fuse") c->opt.vn_fuse = (int)value;
    else if (k == "node_levels") c->opt.node_levels = value != 0;
    else if (k == "x2h_out_fuse") { if (value < 0 || value > 2) return fail("x2h_out_fuse must be 0 (node_out6_kernel), 1 (x2h tail inside its boundary) or 2 (x2h tail always)"); c->opt.x2h_out_fuse = (int)value; }
    else if (k == "stream_chunk") { if (value < 0 || value > 4096) return fail("stream_chunk must be 0 (automatic) .. 4096"); c->opt.stream_chunk_opt = (int)value; }
    else if (k == "after_order") { if (value < 0 || value > 2) return fail("after_order must be 0 (follow-up jobs first), 1 (interleaved) or 2 (linear jobs first)"); c->opt.after_order = (int)value; }
    else if (k == "after_waves") { if (value < 1 || value > 16) return fail("after_waves must be 1..16"); c->opt.after_waves = (int)value; }
    else if (k == "after_lin_wgs") { if (value < 0 || value > 4096) return fail("after_lin_wgs must be 0 (automatic) .. 4096"); c->opt.after_lin_wgs = (int)value; }
    else if (k == "lin_waves") { if (value < 1 || value > 16) return fail("lin_waves must be 1..16"); c->opt.lin_waves = (int)value; }
    else if (k == "stamps") c->stamp_on = (int)value;
    else if (k == "kstamp_sel") c->kstamp_sel = (int)value;
    else if (k == "edge_waves") { if (value < 0 || value > 12) return fail("edge_waves must be 0 (automatic) .. 12"); c->opt.edge_threads = (int)value * 64; }   // 0 = automatic
    else return fail("unknown option " + k);
    hipSetDevice(c->device);
    c->drop_graphs();
    return 0;
}

int64_t shapemol_debug_read(shapemol_ctx *c, const char *name, void *dst, size_t max_bytes) {
    if (!c || !name || !dst) { fail("shapemol_debug_read: null argument"); return -1; }
    const std::string k(name);
    const shapemol_config &g = c->cfg;
    const int64_t N = c->lastN;
    const void *src = nullptr; size_t bytes = 0;
    int64_t dims[8] = {N, c->lastB, c->KP, g.hidden_dim, g.n_heads, g.num_layers, c->capN, c->capB};
    if (k == "dims") { if (max_bytes < sizeof(dims)) return -1; std::memcpy(dst, dims, sizeof(dims)); return sizeof(dims); }
    if (k == "captures") { if (max_bytes < 8) return -1; std::memcpy(dst, &c->n_captures, 8); return 8; }
    if (k == "launch") { if (max_bytes < sizeof(c->launch_rec)) return -1; std::memcpy(dst, c->launch_rec, sizeof(c->launch_rec)); return sizeof(c->launch_rec); }
    if (k == "launch_x2h_out") { if (max_bytes < sizeof(c->x2h_out_rec)) return -1; std::memcpy(dst, c->x2h_out_rec, sizeof(c->x2h_out_rec)); return sizeof(c->x2h_out_rec); }
    if (k == "launch_edge") { if (max_bytes < sizeof(c->edge_rec)) return -1; std::memcpy(dst, c->edge_rec, sizeof(c->edge_rec)); return sizeof(c->edge_rec); }
    if (k == "launch_node") { if (max_bytes < sizeof(c->node_rec)) return -1; std::memcpy(dst, c->node_rec, sizeof(c->node_rec)); return sizeof(c->node_rec); }
    if (k == "nbr") { src = c->nbr; bytes = N * c->KP * 4; }
    else if (k == "ew") { src = c->ew; bytes = N * c->KP * 4; }
    else if (k == "h") { src = c->last_h; bytes = N * g.hidden_dim * 4; }
    else if (k == "x") { src = c->last_x; bytes = N * 3 * 4; }
    else if (k == "h0") { src = c->h_a; bytes = N * g.hidden_dim * 4; }                   // the prologue's outputs: intact after an
    else if (k == "q_x") { src = c->q_x; bytes = N * g.hidden_dim * 4; }                  // evaluation with stop_layer = 1
    else if (k == "pre0") { src = c->pre0; bytes = N * 4 * g.hidden_dim * 4; }
    else if (k == "add0") { src = c->prep[0].add0; bytes = (size_t)c->lastB * 4 * g.hidden_dim * 4; }
    else if (k == "pre") { src = c->preAB; bytes = N * 8 * g.hidden_dim * 4; }
    else if (k == "q") { src = c->q_h; bytes = N * g.hidden_dim * 4; }
    else if (k == "att") { src = c->att; bytes = N * g.hidden_dim * 4; }
    else if (k == "o3") { src = c->o3; bytes = N * 48 * 4; }
    else if (k == "stamps") { src = c->stamps; bytes = 2048 * 8; }
    else if (k == "kstamps") { src = c->kstamps; bytes = (size_t)8 * 16 * 4096 * 8; }
    else if (k == "vn_err") { src = c->status + ST_VN_BARRIER; bytes = 4; }
    else if (k == "mesh_group_flags") { src = c->m_cnt ? c->m_cnt + 4 * c->m_cnt_cap : nullptr; bytes = (size_t)c->m_flag_groups * 4; }
    else if (k == "cfg_stat") { src = c->cfg_stat; bytes = 2 * 4; }
    else if (k == "cfg_group_stat") { src = c->cgs.last_groups > 0 ? c->cgs.stat : nullptr; bytes = (size_t)c->cgs.last_groups * 2 * 4; }
    else if (k == "bnstat") { src = c->bn_acc; bytes = (size_t)g.num_layers * kVnReplicas * 2 * g.n_heads * 8; }
    else { fail("shapemol_debug_read: unknown buffer " + k); return -1; }
    if (!src || bytes > max_bytes) { fail("shapemol_debug_read: buffer unavailable or destination too small"); return -1; }
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) { fail("shapemol_debug_read: copy failed"); return -1; }
    return (int64_t)bytes;
}

/* Diagnostic: the statistic stage of one classifier-free guidance step on the caller's four prediction tensors, under the installed
 * setting: what a chain prepares (run_cfg_prep) and what each of its steps launches (run_cfg_stats on cfg_args), nothing else. */
int shapemol_debug_cfg_stats(shapemol_ctx *c, const float *d_pos_cond, const float *d_pos_uncond, const float *d_v_cond, const float *d_v_uncond,
                             const int64_t *d_batch, int64_t N, int64_t B, void *stream) {
    const std::string me = "shapemol_debug_cfg_stats: ";
    if (!c || !d_pos_cond || !d_pos_uncond || !d_v_cond || !d_v_uncond || !d_batch) return fail(me + "null argument");
    if (N < 1 || B < 1 || B > N || N > (1 << 27) || N * c->cfg.num_classes >= (int64_t)1 << 31) return fail(me + "n_atoms / n_mols out of range");
    if (chain_guide(c) != Guide::Cfg) return fail(me + "no classifier-free guidance setting is installed (or another guidance takes precedence)");
    if (c->cgs.groups > 0 && c->cgs.mols != B)
        return fail(me + "n_mols = " + std::to_string(B) + " but the classifier-free guidance groups cover " + std::to_string(c->cgs.mols) + " molecules");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, B)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (run_cfg_prep(c, s, d_batch, N, B)) return 1;
    CfgArgs a = cfg_args(c, N);
    a.pos_c = d_pos_cond; a.pos_u = d_pos_uncond; a.v_c = d_v_cond; a.v_u = d_v_uncond;
    return run_cfg_stats(c, s, a);
}

/* Diagnostic: the exact three-way bf16 split the packers apply to every weight (and the kernels, with the same arithmetic, to every
 * activation): pieces[0..2] = hi, mid, lo bit patterns, x == float(hi) + float(mid) + float(lo) exactly for |x| >= 2^-110. */
void shapemol_debug_split_exact(float x, uint16_t *pieces) {
    uint16_t p[3];
    split3_host(x, p);
    pieces[0] = p[0]; pieces[1] = p[1]; pieces[2] = p[2];
}

int shapemol_set_knn_pins(shapemol_ctx *c, const int32_t *h_off, int32_t n_steps, const int32_t *h_atom, const int32_t *h_nbr, int64_t n_pins, int32_t k) {
    if (!c) return fail("shapemol_set_knn_pins: null context");
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();
    HIPCHK(hipDeviceSynchronize());
    c->mem_pins.release();
    c->n_pins = 0; c->pin_steps = 0; c->pin_k = 0;
    if (n_pins <= 0) return 0;
    if (!h_off || !h_atom || !h_nbr || n_steps < 1 || k < 1 || k > c->KP) return fail("shapemol_set_knn_pins: bad arguments");
    if (h_off[0] != 0 || h_off[n_steps] != n_pins) return fail("shapemol_set_knn_pins: offsets do not cover the pins");
    for (int i = 0; i < n_steps; ++i) if (h_off[i + 1] < h_off[i]) return fail("shapemol_set_knn_pins: offsets must not decrease");
    HIPCHK(c->mem_pins.alloc(&c->pin_off, (size_t)(n_steps + 1) * 4)); HIPCHK(c->mem_pins.alloc(&c->pin_atom, (size_t)n_pins * 4));
    HIPCHK(c->mem_pins.alloc(&c->pin_nbr, (size_t)n_pins * k * 4));
    HIPCHK(hipMemcpy(c->pin_off, h_off, (size_t)(n_steps + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->pin_atom, h_atom, (size_t)n_pins * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->pin_nbr, h_nbr, (size_t)n_pins * k * 4, hipMemcpyHostToDevice));
    c->n_pins = n_pins; c->pin_steps = n_steps; c->pin_k = k;
    return 0;
}

int shapemol_set_cfg(shapemol_ctx *c, double guide_stren, int32_t threshold_type, double p, const double *h_bounds,
                     float *d_pos_uncond_traj, float *d_v_uncond_traj) {
    if (!c) return fail("shapemol_set_cfg: null ctx");
    if (!(guide_stren == guide_stren) || threshold_type < CFG_NONE || threshold_type > CFG_RESCALE || !(p == p))
        return fail("shapemol_set_cfg: bad arguments");
    c->cfg_w = guide_stren; c->cfg_type = guide_stren != 0.0 ? threshold_type : 0; c->cfg_p = guide_stren != 0.0 ? p : 0.0;
    c->cfg_has_bounds = guide_stren != 0.0 && h_bounds != nullptr;
    for (int k = 0; k < 3; ++k) {
        c->cfg_lo[k] = c->cfg_has_bounds ? (float)h_bounds[2 * k] : 0.f;
        c->cfg_hi[k] = c->cfg_has_bounds ? (float)h_bounds[2 * k + 1] : 0.f;
    }
    c->cfg_tr_pos_u = guide_stren != 0.0 ? d_pos_uncond_traj : nullptr;
    c->cfg_tr_v_u = guide_stren != 0.0 ? d_v_uncond_traj : nullptr;
    return 0;
}

int shapemol_set_cfg_groups(shapemol_ctx *c, int32_t n_groups, const int64_t *h_mol_off, const double *h_guide_stren, int32_t threshold_type,
                            double p, const double *h_bounds, float *d_pos_uncond_traj, float *d_v_uncond_traj) {
    const std::string me = "shapemol_set_cfg_groups: ";
    if (!c) return fail(me + "null ctx");
    if (n_groups < 0) return fail(me + "n_groups < 0");
    if (n_groups > kCfgMaxGroups) return fail(me + std::to_string(n_groups) + " groups, at most " + std::to_string(kCfgMaxGroups) + " per chain");
    bool any = false;
    if (n_groups > 0) {
        if (!h_mol_off || !h_guide_stren) return fail(me + "offsets / strengths missing");
        if (threshold_type < CFG_NONE || threshold_type > CFG_RESCALE || !(p == p)) return fail(me + "bad threshold type or p");
        if (h_mol_off[0] != 0) return fail(me + "group 0: the molecule offsets must start at 0");
        for (int g = 0; g < n_groups; ++g) {
            const std::string grp = me + "group " + std::to_string(g) + ": ";
            if (h_mol_off[g + 1] < h_mol_off[g]) return fail(grp + "the molecule offsets decrease");
            if (!std::isfinite(h_guide_stren[g])) return fail(grp + "the guidance strength is not finite");
            any = any || h_guide_stren[g] != 0.0;
        }
        if (h_mol_off[n_groups] > (1 << 27)) return fail(me + "too many molecules");
    }
    HIPCHK(hipSetDevice(c->device));
    CfgGroupSet &gs = c->cgs;
    gs.groups = 0; gs.mols = 0; gs.type = 0; gs.p = 0.0; gs.tr_pos_u = gs.tr_v_u = nullptr;
    if (!any) return 0;        // no group, or every strength 0: the unguided chain
    std::vector<CfgGroup> rows((size_t)n_groups + 1, CfgGroup{});
    for (int g = 0; g <= n_groups; ++g) rows[g].mol0 = (int)h_mol_off[g];
    for (int g = 0; g < n_groups; ++g) {
        CfgGroup &r = rows[g];
        const double w = h_guide_stren[g];
        r.w1 = (float)(1.0 + w); r.w = (float)w;
        r.type = w != 0.0 ? threshold_type : CFG_NONE;
        const double *b = h_bounds ? h_bounds + (size_t)g * 6 : nullptr;
        r.has_box = w != 0.0 && b && b[0] == b[0];      // (a NaN row: no clamp for this group)
        for (int k = 0; k < 3; ++k) { r.lo[k] = r.has_box ? (float)b[2 * k] : 0.f; r.hi[k] = r.has_box ? (float)b[2 * k + 1] : 0.f; }
    }
    // a chain that reads the rows may still be running: wait for it before they are overwritten (or their block replaced)
    if (gs.stream_set && hipStreamSynchronize(gs.stream) != hipSuccess) hipDeviceSynchronize();
    if (n_groups > gs.cap) {
        c->drop_graphs();                        // the captured steps point into the old block
        gs.stat = nullptr; gs.hist = nullptr; gs.last_groups = 0;
        const size_t rb = ((size_t)(n_groups + 1) * sizeof(CfgGroup) + 255) / 256 * 256, sb = ((size_t)n_groups * 2 * sizeof(float) + 255) / 256 * 256;
        HIPCHK(grow(gs.mem, {dev_buf(&gs.rows, rb + sb + (size_t)n_groups * 2 * kCfgHistWords * sizeof(unsigned))}, gs.cap, n_groups));
        unsigned char *blk = reinterpret_cast<unsigned char *>(gs.rows);
        gs.stat = reinterpret_cast<float *>(blk + rb); gs.hist = reinterpret_cast<unsigned *>(blk + rb + sb);
    }
    HIPCHK(hipMemcpy(gs.rows, rows.data(), rows.size() * sizeof(CfgGroup), hipMemcpyHostToDevice));
    gs.groups = n_groups; gs.mols = h_mol_off[n_groups];
    gs.type = threshold_type; gs.p = threshold_type != CFG_NONE ? p : 0.0;
    gs.tr_pos_u = d_pos_uncond_traj; gs.tr_v_u = d_v_uncond_traj;
    return 0;
}

static int status_message(const int32_t (&f)[8]) {
    if (f[ST_BATCH]) return fail("batch vector is not sorted ascending or names a molecule >= n_mols; results are invalid");
    if (f[ST_ATOM_TYPE]) return fail("an atom type is outside [0, num_classes); results are invalid");
    if (f[ST_TIME]) return fail("a time step is outside [0, num_timesteps); results are invalid");
    if (f[ST_SPAN]) return fail("a molecule is larger than the max_mol_atoms hint says (folded coordinate update / fused graph kernel); results are invalid");
    if (f[ST_RANGE]) return fail("an activation left the fp16 range of the two-piece f16 node kernels (|x| >= 6e4 or NaN); results are invalid: set option node_f16 = 0 (exactly split bf16 kernels)");
    if (f[ST_VN_BARRIER]) return fail("grid barrier of the fused coordinate update timed out (workgroups not co-resident); results are invalid");
    if (f[ST_MESH]) return fail("mesh shape guidance: fewer than 3 atoms lie inside the mesh and > 0.4 from the cloud (none at all, or "
                                "fewer than 3 while atoms are to be pulled); the reference raises ValueError from its KD-tree here");
    return 0;
}

int shapemol_status(shapemol_ctx *c, int32_t *flags_out) {
    if (!c) return fail("shapemol_status: null ctx");
    int32_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (c->status) HIPCHK(hipMemcpy(f, c->status, sizeof(f), hipMemcpyDeviceToHost));
    if (flags_out) std::memcpy(flags_out, f, sizeof(f));
    return status_message(f);
}

int shapemol_status_stream(shapemol_ctx *c, int32_t *flags_out, void *stream) {
    if (!c) return fail("shapemol_status_stream: null ctx");
    int32_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (c->status) HIPCHK(hipMemcpyAsync(f, c->status, sizeof(f), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags_out) std::memcpy(flags_out, f, sizeof(f));
    return status_message(f);
}

int shapemol_profile_begin(shapemol_ctx *c) {
    if (!c) return fail("shapemol_profile_begin: null ctx");
    for (auto &r : c->prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    c->prof.clear();
    c->prof_on = true;
    return 0;
}

int shapemol_profile_end(shapemol_ctx *c, char (*names)[32], double *total_ms, int64_t *launches, int cap) {
    if (!c) { fail("shapemol_profile_end: null ctx"); return -1; }
    c->prof_on = false;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    std::vector<std::string> order;
    std::map<std::string, std::pair<double, int64_t>> acc;
    for (auto &r : c->prof) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        if (!acc.count(r.name)) order.push_back(r.name);
        acc[r.name].first += ms; acc[r.name].second += 1;
        hipEventDestroy(r.e0); hipEventDestroy(r.e1);
    }
    c->prof.clear();
    int n = 0;
    for (auto &nm : order) {
        if (n >= cap) break;
        std::snprintf(names[n], 32, "%s", nm.c_str());
        total_ms[n] = acc[nm].first; launches[n] = acc[nm].second; ++n;
    }
    return n;
}

}  // extern "C"
