// C ABI of the Gaussian similarity of molecules (include/shapemol_hip.h, shapemol_sim_*): shape and electrostatic overlap
// integrals and their Tanimoto / Carbo scores at a fixed pose, and the rigid overlay that maximises the shape overlap, for a
// list of pairs from two packed sets, on the device.  The arithmetic, the kernels and the host plan: sm_mol_sim.h.
#include "../../include/shapemol_hip.h"
#include "sm_mol_sim.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <cstring>
#include <string>
#include <vector>

struct shapemol_sim_ctx {
    int device = 0;
    MsimPlan plan;                        // of the last call
    std::vector<unsigned char> up;        // the upload's host image: per-atom parameters, term tables, jobs, molecules, pairs
    unsigned char *d_in = nullptr; int64_t cap_in = 0; DevList mem_in;       // the upload, bytes (sm_devmem.h)
    double *d_ws = nullptr; int64_t cap_ws = 0; DevList mem_ws;              // integrals, start results, overlaid copies: doubles
};

namespace {

MsimSet set_of(int64_t n_mols, const int64_t *off, const double *u, const double *v) { return {n_mols, off, u, v}; }

// the per-atom parameters of both sets and the term tables, behind each other in the image
struct ParamOffsets { size_t u[2], v[2], cA, cB; };

ParamOffsets put_params(std::vector<unsigned char> &img, int mode, const MsimPlan &pl, const MsimSet &a, const MsimSet &b, int K, const double *cA,
                        const double *cB) {
    ParamOffsets o{};
    const MsimSet *sets[2] = {&a, &b};
    for (int s = 0; s < 2; ++s) {
        o.u[s] = put(img, sets[s]->u, (size_t)pl.n_atoms[s]);
        o.v[s] = mode == MSIM_SHAPE ? put(img, sets[s]->v, (size_t)pl.n_atoms[s]) : o.u[s];
    }
    o.cA = put(img, cA, mode == MSIM_ESP ? (size_t)K : 0);
    o.cB = put(img, cB, mode == MSIM_ESP ? (size_t)K : 0);
    return o;
}

template <int MODE> void launch_integrals(MsimIntArgs a, const unsigned char *d_in, const size_t (&o_jobs)[2], const std::vector<MsimJob> (&jobs)[2], hipStream_t s) {
    if (!jobs[0].empty()) {
        a.jobs = reinterpret_cast<const MsimJob *>(d_in + o_jobs[0]);
        hipLaunchKernelGGL((msim_integral_kernel<kMsimWaveAtoms, MODE>), dim3((unsigned)jobs[0].size()), dim3(kMsimWaveAtoms), 0, s, a);
    }
    if (!jobs[1].empty()) {
        a.jobs = reinterpret_cast<const MsimJob *>(d_in + o_jobs[1]);
        hipLaunchKernelGGL((msim_integral_kernel<kMsimMaxAtoms, MODE>), dim3((unsigned)jobs[1].size()), dim3(kMsimMaxAtoms), 0, s, a);
    }
}

}  // namespace

extern "C" {

int shapemol_sim_sizes(int64_t *out, int32_t n) {
    const int64_t v[6] = {kMsimWaveAtoms, kMsimMaxAtoms, kMsimMaxTerms, kMsimMaxStarts, kMsimMaxIter, kMsimMaxPairs};
    for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
    return 6;
}

int shapemol_sim_check(int32_t mode, int64_t n_mols_a, const int64_t *h_off_a, const double *h_u_a, const double *h_v_a, int64_t n_mols_b,
                       const int64_t *h_off_b, const double *h_u_b, const double *h_v_b, int64_t n_pairs, const int64_t *h_pairs, int32_t n_terms,
                       const double *h_term_a, const double *h_term_b, int32_t *h_forms) {
    MsimPlan pl;
    const std::string e = msim_plan(mode, set_of(n_mols_a, h_off_a, h_u_a, h_v_a), set_of(n_mols_b, h_off_b, h_u_b, h_v_b), n_pairs, h_pairs, n_terms,
                                    h_term_a, h_term_b, &pl);
    if (!e.empty()) return sm_fail(e);
    if (h_forms) std::memcpy(h_forms, pl.form.data(), pl.form.size() * sizeof(int));
    return 0;
}

int shapemol_sim_create(int device, shapemol_sim_ctx **out) {
    if (!out) return sm_fail("shapemol_sim_create: null argument");
    if (sm_open_device(device, "shapemol_sim_create")) return 1;
    shapemol_sim_ctx *c = new shapemol_sim_ctx;
    c->device = device;
    *out = c;
    return 0;
}

void shapemol_sim_destroy(shapemol_sim_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                              // the lists free their buffers
}

int shapemol_sim_score(shapemol_sim_ctx *c, int32_t mode, int32_t metric, int64_t n_mols_a, const int64_t *h_off_a, const double *d_pos_a,
                       const double *h_u_a, const double *h_v_a, int64_t n_mols_b, const int64_t *h_off_b, const double *d_pos_b, const double *h_u_b,
                       const double *h_v_b, int64_t n_pairs, const int64_t *h_pairs, int32_t n_terms, const double *h_term_a, const double *h_term_b,
                       double *d_out, int32_t *d_flags, void *stream) {
    if (!c) return sm_fail("shapemol_sim_score: null context");
    if (!d_pos_a || !d_pos_b || !d_out || !d_flags) return sm_fail("shapemol_sim_score: null argument");
    if (metric != MSIM_TANIMOTO && metric != MSIM_CARBO) return sm_fail("molecule similarity: unknown metric " + std::to_string(metric));
    const MsimSet sa = set_of(n_mols_a, h_off_a, h_u_a, h_v_a), sb = set_of(n_mols_b, h_off_b, h_u_b, h_v_b);
    // a call before this one has synchronised its stream before it returned: the host image is free to be rewritten
    const std::string err = msim_plan(mode, sa, sb, n_pairs, h_pairs, n_terms, h_term_a, h_term_b, &c->plan);
    if (!err.empty()) return sm_fail(err);
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const MsimPlan &pl = c->plan;
    const int Ma = (int)n_mols_a, Mb = (int)n_mols_b, P = (int)n_pairs;
    std::vector<MsimJob> jobs[2];
    msim_self_jobs(pl, jobs);
    msim_cross_jobs(pl, 0, Ma + Mb, jobs);
    std::vector<unsigned char> &img = c->up;
    img.clear();
    const ParamOffsets po = put_params(img, mode, pl, sa, sb, n_terms, h_term_a, h_term_b);
    const size_t o_jobs[2] = {put(img, jobs[0].data(), jobs[0].size()), put(img, jobs[1].data(), jobs[1].size())};
    const size_t o_pairs = put(img, pl.pairs.data(), pl.pairs.size());
    SMCHK(grow(c->mem_in, {dev_buf(&c->d_in, img.size())}, c->cap_in, (int64_t)img.size()));
    const int64_t n_ws = (int64_t)Ma + Mb + P;
    SMCHK(grow(c->mem_ws, {dev_buf(&c->d_ws, (size_t)n_ws * sizeof(double))}, c->cap_ws, n_ws));
    SMCHK(hipMemcpyAsync(c->d_in, img.data(), img.size(), hipMemcpyHostToDevice, s));
    MsimIntArgs a{};
    a.pos[0] = d_pos_a; a.pos[1] = d_pos_b; a.pos[2] = d_pos_a;
    for (int k = 0; k < 2; ++k) {
        a.u[k] = reinterpret_cast<const double *>(c->d_in + po.u[k]);
        a.v[k] = reinterpret_cast<const double *>(c->d_in + po.v[k]);
    }
    a.cA = reinterpret_cast<const double *>(c->d_in + po.cA); a.cB = reinterpret_cast<const double *>(c->d_in + po.cB);
    a.K = mode == MSIM_ESP ? n_terms : 0;
    a.out = c->d_ws;
    if (mode == MSIM_SHAPE) launch_integrals<MSIM_SHAPE>(a, c->d_in, o_jobs, jobs, s);
    else launch_integrals<MSIM_ESP>(a, c->d_in, o_jobs, jobs, s);
    MsimFinishArgs f{};
    f.pairs = reinterpret_cast<const MsimPair *>(c->d_in + o_pairs);
    f.n_pairs = P; f.n_mols_a = Ma; f.n_mols_b = Mb; f.metric = metric;
    f.integ = c->d_ws; f.out = d_out; f.flags = d_flags;
    hipLaunchKernelGGL(msim_score_finish_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, f);
    SMCHK(hipGetLastError());
    SMCHK(hipStreamSynchronize(s));
    return 0;
}

int shapemol_sim_align(shapemol_sim_ctx *c, int64_t n_mols_a, const int64_t *h_off_a, const double *d_pos_a, const double *h_alpha_a,
                       const double *h_p_a, int64_t n_mols_b, const int64_t *h_off_b, const double *d_pos_b, const double *h_alpha_b,
                       const double *h_p_b, int64_t n_pairs, const int64_t *h_pairs, int32_t include_given, int32_t max_iter, double gtol,
                       double *d_out, double *d_rot, double *d_trans, int32_t *d_info, double *d_aligned, void *stream) {
    if (!c) return sm_fail("shapemol_sim_align: null context");
    if (!d_pos_a || !d_pos_b || !d_out || !d_rot || !d_trans || !d_info) return sm_fail("shapemol_sim_align: null argument");
    if (max_iter < 0 || max_iter > kMsimMaxIter) return sm_fail("molecule similarity: the iteration cap must lie in 0.." + std::to_string(kMsimMaxIter));
    if (!(gtol >= 0.0) || !std::isfinite(gtol)) return sm_fail("molecule similarity: the stopping threshold must be finite and not negative");
    const MsimSet sa = set_of(n_mols_a, h_off_a, h_alpha_a, h_p_a), sb = set_of(n_mols_b, h_off_b, h_alpha_b, h_p_b);
    const std::string err = msim_plan(MSIM_SHAPE, sa, sb, n_pairs, h_pairs, 0, nullptr, nullptr, &c->plan);
    if (!err.empty()) return sm_fail(err);
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const MsimPlan &pl = c->plan;
    const int Ma = (int)n_mols_a, Mb = (int)n_mols_b, P = (int)n_pairs, S = include_given ? kMsimMaxStarts : kMsimStarts;
    std::vector<MsimJob> self[2], cross[2];
    msim_self_jobs(pl, self);
    msim_cross_jobs(pl, 2, Ma + Mb, cross);
    if (include_given) msim_cross_jobs(pl, 0, Ma + Mb + P, cross);
    std::vector<unsigned char> &img = c->up;
    img.clear();
    const ParamOffsets po = put_params(img, MSIM_SHAPE, pl, sa, sb, 0, nullptr, nullptr);
    const size_t o_self[2] = {put(img, self[0].data(), self[0].size()), put(img, self[1].data(), self[1].size())};
    const size_t o_cross[2] = {put(img, cross[0].data(), cross[0].size()), put(img, cross[1].data(), cross[1].size())};
    const size_t o_pairs = put(img, pl.pairs.data(), pl.pairs.size());
    const size_t o_mol[2] = {put(img, pl.mol[0].data(), pl.mol[0].size()), put(img, pl.mol[1].data(), pl.mol[1].size())};
    const size_t o_list[2] = {put(img, pl.list[0].data(), pl.list[0].size()), put(img, pl.list[1].data(), pl.list[1].size())};
    SMCHK(grow(c->mem_in, {dev_buf(&c->d_in, img.size())}, c->cap_in, (int64_t)img.size()));
    const int64_t n_integ = (int64_t)Ma + Mb + 2 * (int64_t)P, n_starts = (int64_t)P * S * kMsimStartDoubles;
    const int64_t n_ws = n_integ + n_starts + (d_aligned ? 0 : 3 * pl.n_aligned);
    SMCHK(grow(c->mem_ws, {dev_buf(&c->d_ws, (size_t)n_ws * sizeof(double))}, c->cap_ws, n_ws));
    SMCHK(hipMemcpyAsync(c->d_in, img.data(), img.size(), hipMemcpyHostToDevice, s));
    double *d_integ = c->d_ws, *d_starts = c->d_ws + n_integ, *aligned = d_aligned ? d_aligned : c->d_ws + n_integ + n_starts;
    MsimIntArgs a{};
    a.pos[0] = d_pos_a; a.pos[1] = d_pos_b; a.pos[2] = aligned;
    for (int k = 0; k < 2; ++k) {
        a.u[k] = reinterpret_cast<const double *>(c->d_in + po.u[k]);
        a.v[k] = reinterpret_cast<const double *>(c->d_in + po.v[k]);
    }
    a.out = d_integ;
    launch_integrals<MSIM_SHAPE>(a, c->d_in, o_self, self, s);
    MsimAlignArgs g{};
    g.pos_a = d_pos_a; g.pos_b = d_pos_b;
    for (int k = 0; k < 2; ++k) { g.u[k] = a.u[k]; g.v[k] = a.v[k]; }
    g.mol_a = reinterpret_cast<const MsimMol *>(c->d_in + o_mol[0]); g.mol_b = reinterpret_cast<const MsimMol *>(c->d_in + o_mol[1]);
    g.pairs = reinterpret_cast<const MsimPair *>(c->d_in + o_pairs);
    g.n_starts = S; g.max_iter = max_iter; g.gtol = gtol;
    g.self = d_integ; g.n_mols_a = Ma; g.starts = d_starts;
    if (!pl.list[0].empty()) {
        g.list = reinterpret_cast<const int *>(c->d_in + o_list[0]);
        hipLaunchKernelGGL(msim_align_kernel<kMsimWaveAtoms>, dim3((unsigned)(pl.list[0].size() * S)), dim3(kMsimWaveAtoms), 0, s, g);
    }
    if (!pl.list[1].empty()) {
        g.list = reinterpret_cast<const int *>(c->d_in + o_list[1]);
        hipLaunchKernelGGL(msim_align_kernel<kMsimMaxAtoms>, dim3((unsigned)(pl.list[1].size() * S)), dim3(kMsimMaxAtoms), 0, s, g);
    }
    MsimFinishArgs f{};
    f.pairs = g.pairs; f.mol_a = g.mol_a;
    f.n_pairs = P; f.n_mols_a = Ma; f.n_mols_b = Mb; f.n_starts = S; f.metric = MSIM_TANIMOTO; f.include_given = include_given != 0;
    f.integ = d_integ; f.starts = d_starts; f.pos_a = d_pos_a;
    f.out = d_out; f.flags = d_info; f.rot = d_rot; f.trans = d_trans; f.aligned = aligned;
    hipLaunchKernelGGL(msim_pick_kernel, dim3((unsigned)P), dim3(64), 0, s, f);
    launch_integrals<MSIM_SHAPE>(a, c->d_in, o_cross, cross, s);
    hipLaunchKernelGGL(msim_align_finish_kernel, dim3((unsigned)P), dim3(64), 0, s, f);
    SMCHK(hipGetLastError());
    SMCHK(hipStreamSynchronize(s));
    return 0;
}

int shapemol_sim_debug_fill(shapemol_sim_ctx *c, int32_t byte, void *stream) {
    if (!c) return sm_fail("shapemol_sim_debug_fill: null context");
    SMCHK(hipSetDevice(c->device));
    if (c->cap_in) SMCHK(hipMemsetAsync(c->d_in, byte, (size_t)c->cap_in, (hipStream_t)stream));
    if (c->cap_ws) SMCHK(hipMemsetAsync(c->d_ws, byte, (size_t)c->cap_ws * sizeof(double), (hipStream_t)stream));
    SMCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
