// C ABI of the geometry scores of sampled molecules (include/shapemol_hip.h, shapemol_eval_*): bond orders from distance
// thresholds, stable atoms and molecules, pair-distance histograms and class counts for every frame of a packed batch, on the
// device.  The kernel: sm_mol_eval.h; the arithmetic and the host plan: sm_mol_rule.h; the upload and the launch: sm_mol_upload.h.
#include "../../include/shapemol_hip.h"
#include "sm_mol_eval.h"
#include "sm_mol_upload.h"

struct shapemol_eval_ctx {
    int device = 0;
    MolInput in{"molecule evaluation"};   // the plan and the upload, the context's only device buffer
};

extern "C" {

int shapemol_eval_sizes(int64_t *out, int32_t n) {
    const int64_t v[6] = {kMolWaveAtoms, kMevalMaxAtoms, kMolMaxElements, kMolMaxClasses, kMolMaxEdges, kMolThreads};
    for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
    return 6;
}

int shapemol_eval_check(int64_t n_frames, int64_t n_mols, const int64_t *h_off, int32_t n_elements, int32_t n_classes, const int32_t *h_class_slot,
                        const double *h_cc_edges, int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all, double all_cut,
                        int32_t *h_forms) {
    MolPlan pl;
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
    const std::string err = meval_plan(n_frames, n_mols, h_off, n_elements, n_classes, h_class_slot, h_cc_edges, n_cc, cc_cut, h_all_edges, n_all, all_cut, &c->in.plan);
    if (!err.empty()) return sm_fail(err);
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    MevalArgs a{};
    if (mol_upload(c->in, s, n_frames, n_mols, d_pos, d_classes, classes_int64, n_elements, h_thresholds, carbon_slot, n_classes, h_class_slot, h_cc_edges,
                   n_cc, cc_cut, h_all_edges, n_all, all_cut, h_allowed, (size_t)n_elements, &a.allowed, a.b, a.r))
        return 1;
    if (mol_zero_counts(a.o, d_hist_cc, d_hist_all, d_class_counts, a.b, a.r, s)) return 1;
    a.hs = hs != 0;
    a.nr_bonds = d_nr_bonds; a.n_stable = d_n_stable; a.mol_stable = d_mol_stable;
    mol_launch(meval_kernel<64>, meval_kernel<kMolThreads>, c->in, a, s);
    return mol_finish(c->in, n_classes, s);
}

int shapemol_eval_debug_fill(shapemol_eval_ctx *c, int32_t byte, void *stream) {
    if (!c) return sm_fail("shapemol_eval_debug_fill: null context");
    SMCHK(hipSetDevice(c->device));
    if (c->in.cap_in) SMCHK(hipMemsetAsync(c->in.d_in, byte, (size_t)c->in.cap_in, (hipStream_t)stream));
    SMCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
