// C ABI of the geometry scores of sampled molecules (include/shapemol_hip.h, shapemol_eval_*): bond orders from distance
// thresholds, stable atoms and molecules, pair-distance histograms and class counts for every frame of a packed batch, on the
// device.  The arithmetic, the kernel and the host plan: sm_mol_eval.h.
#include "../../include/shapemol_hip.h"
#include "sm_mol_eval.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <cstring>
#include <string>
#include <vector>

struct shapemol_eval_ctx {
    int device = 0;
    MevalPlan plan;                       // of the last call (the upload reads its image until the call's synchronise)
    std::vector<unsigned char> up;        // the upload's host image: rule tables, bin edges, molecules, job lists, class table
    unsigned char *d_in = nullptr; int64_t cap_in = 0; DevList mem_in;       // the upload, bytes (sm_devmem.h)
};

namespace {

template <typename T> size_t put(std::vector<unsigned char> &img, const T *src, size_t count) {      // -> the offset, 8-aligned
    const size_t o = (img.size() + 7) / 8 * 8;
    img.resize(o + count * sizeof(T));
    if (count) std::memcpy(img.data() + o, src, count * sizeof(T));
    return o;
}

}  // namespace

extern "C" {

int shapemol_eval_sizes(int64_t *out, int32_t n) {
    const int64_t v[6] = {kMevalWaveAtoms, kMevalMaxAtoms, kMevalMaxElements, kMevalMaxClasses, kMevalMaxEdges, kMevalThreads};
    for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
    return 6;
}

int shapemol_eval_check(int64_t n_frames, int64_t n_mols, const int64_t *h_off, int32_t n_elements, int32_t n_classes, const int32_t *h_class_slot,
                        const double *h_cc_edges, int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all, double all_cut,
                        int32_t *h_forms) {
    MevalPlan pl;
    const std::string e = meval_plan(n_frames, n_mols, h_off, n_elements, n_classes, h_class_slot, h_cc_edges, n_cc, cc_cut, h_all_edges, n_all, all_cut, &pl);
    if (!e.empty()) return sm_fail(e);
    if (h_forms) std::memcpy(h_forms, pl.form.data(), pl.form.size() * sizeof(int));
    return 0;
}

int shapemol_eval_create(int device, shapemol_eval_ctx **out) {
    if (!out) return sm_fail("shapemol_eval_create: null argument");
    if (sm_open_device(device, "shapemol_eval_create")) return 1;
    shapemol_eval_ctx *c = new shapemol_eval_ctx;
    c->device = device;
    *out = c;
    return 0;
}

void shapemol_eval_destroy(shapemol_eval_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                              // the list frees its buffer
}

int shapemol_eval_run(shapemol_eval_ctx *c, int64_t n_frames, int64_t n_mols, const int64_t *h_off, const float *d_pos, const void *d_classes,
                      int32_t classes_int64, int32_t n_elements, const double *h_thresholds, const double *h_allowed, int32_t carbon_slot,
                      int32_t n_classes, const int32_t *h_class_slot, const double *h_cc_edges, int32_t n_cc, double cc_cut,
                      const double *h_all_edges, int32_t n_all, double all_cut, int32_t hs, int32_t *d_nr_bonds, int32_t *d_n_stable,
                      uint8_t *d_mol_stable, int64_t *d_hist_cc, int64_t *d_hist_all, int64_t *d_class_counts, void *stream) {
    if (!c) return sm_fail("shapemol_eval_run: null context");
    if (!d_pos || !d_classes || !h_thresholds || !h_allowed || !d_nr_bonds || !d_n_stable || !d_mol_stable || !d_hist_cc || !d_hist_all || !d_class_counts)
        return sm_fail("shapemol_eval_run: null argument");
    // a run before this one has synchronised its stream before it returned: the host image is free to be rewritten
    const std::string err = meval_plan(n_frames, n_mols, h_off, n_elements, n_classes, h_class_slot, h_cc_edges, n_cc, cc_cut, h_all_edges, n_all, all_cut, &c->plan);
    if (!err.empty()) return sm_fail(err);
    if (carbon_slot < -1 || carbon_slot >= n_elements) return sm_fail("molecule evaluation: the carbon slot lies outside the rule");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const MevalPlan &pl = c->plan;
    const int E = n_elements, C = n_classes, B = (int)n_mols, F = (int)n_frames;
    unsigned char slot[kMevalMaxClasses];
    for (int k = 0; k < C; ++k) slot[k] = (unsigned char)h_class_slot[k];
    const int zero = 0;
    std::vector<unsigned char> &img = c->up;
    img.clear();
    const size_t o_thr = put(img, h_thresholds, (size_t)3 * E * E), o_al = put(img, h_allowed, (size_t)E);
    const size_t o_cc = put(img, h_cc_edges, (size_t)n_cc), o_all = put(img, h_all_edges, (size_t)n_all);
    const size_t o_mol = put(img, pl.mol.data(), pl.mol.size());
    const size_t o_wave = put(img, pl.wave.jobs.data(), pl.wave.jobs.size()), o_block = put(img, pl.block.jobs.data(), pl.block.jobs.size());
    const size_t o_slot = put(img, slot, (size_t)C), o_bad = put(img, &zero, 1);
    SMCHK(grow(c->mem_in, {dev_buf(&c->d_in, img.size())}, c->cap_in, (int64_t)img.size()));
    SMCHK(hipMemcpyAsync(c->d_in, img.data(), img.size(), hipMemcpyHostToDevice, s));
    SMCHK(hipMemsetAsync(d_hist_cc, 0, (size_t)F * (n_cc + 1) * 8, s));
    SMCHK(hipMemsetAsync(d_hist_all, 0, (size_t)F * (n_all + 1) * 8, s));
    SMCHK(hipMemsetAsync(d_class_counts, 0, (size_t)F * C * 8, s));
    MevalArgs a{};
    a.pos = d_pos; a.cls = d_classes; a.cls64 = classes_int64 != 0;
    a.N = pl.N; a.F = F; a.B = B;
    a.mol = reinterpret_cast<const MevalMol *>(c->d_in + o_mol);
    a.thr = reinterpret_cast<const double *>(c->d_in + o_thr);
    a.allowed = reinterpret_cast<const double *>(c->d_in + o_al);
    a.slot = c->d_in + o_slot;
    a.E = E; a.C = C; a.carbon = carbon_slot; a.hs = hs != 0;
    a.cc_edges = reinterpret_cast<const double *>(c->d_in + o_cc); a.all_edges = reinterpret_cast<const double *>(c->d_in + o_all);
    a.n_cc = n_cc; a.n_all = n_all; a.cc_cut = cc_cut; a.all_cut = all_cut;
    a.nr_bonds = d_nr_bonds; a.n_stable = d_n_stable; a.mol_stable = d_mol_stable;
    a.hist_cc = reinterpret_cast<unsigned long long *>(d_hist_cc); a.hist_all = reinterpret_cast<unsigned long long *>(d_hist_all);
    a.cls_counts = reinterpret_cast<unsigned long long *>(d_class_counts);
    a.bad = reinterpret_cast<int *>(c->d_in + o_bad);
    if (pl.wave.gx) {
        a.jobs = reinterpret_cast<const int *>(c->d_in + o_wave); a.n_jobs = (int)pl.wave.jobs.size(); a.gx = pl.wave.gx; a.iters = pl.wave.iters;
        hipLaunchKernelGGL(meval_kernel<64>, dim3((unsigned)((int64_t)pl.wave.gx * F)), dim3(kMevalThreads), 0, s, a);
    }
    if (pl.block.gx) {
        a.jobs = reinterpret_cast<const int *>(c->d_in + o_block); a.n_jobs = (int)pl.block.jobs.size(); a.gx = pl.block.gx; a.iters = pl.block.iters;
        hipLaunchKernelGGL(meval_kernel<kMevalThreads>, dim3((unsigned)((int64_t)pl.block.gx * F)), dim3(kMevalThreads), 0, s, a);
    }
    SMCHK(hipGetLastError());
    int bad = 0;
    SMCHK(hipMemcpyAsync(&bad, c->d_in + o_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    SMCHK(hipStreamSynchronize(s));
    if (bad) return sm_fail("molecule evaluation: " + std::to_string(bad) + " atom(s) have a class outside the " + std::to_string(C) + " classes; the outputs are not valid");
    return 0;
}

int shapemol_eval_debug_fill(shapemol_eval_ctx *c, int32_t byte, void *stream) {
    if (!c) return sm_fail("shapemol_eval_debug_fill: null context");
    SMCHK(hipSetDevice(c->device));
    if (c->cap_in) SMCHK(hipMemsetAsync(c->d_in, byte, (size_t)c->cap_in, (hipStream_t)stream));
    SMCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
