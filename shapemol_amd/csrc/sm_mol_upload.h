// What a run of the geometry scores (mol_eval.hip) and of the bond graphs (mol_graph.hip) do alike on the host: the one upload
// of a call -- rule tables, bin edges, molecules, job lists, class table, the `bad` word -- the argument blocks of sm_mol_rule.h
// filled from its offsets, the launch of a kernel in its two forms, and the end of the call.  Host only.
#pragma once
#include "sm_mol_rule.h"
#include "sm_devmem.h"
#include "sm_host.h"

struct MolInput {
    const char *what;                     // the feature, as its refusals name it
    explicit MolInput(const char *w) : what(w) {}
    MolPlan plan;                         // of the last call (the upload reads its image until the call's synchronise)
    std::vector<unsigned char> up;        // the upload's host image
    unsigned char *d_in = nullptr; int64_t cap_in = 0; DevList mem_in;       // the upload, bytes (sm_devmem.h)
    size_t o_wave = 0, o_block = 0, o_bad = 0;                               // the two job lists and the `bad` word in it
};

namespace {

// The host arrays of a planned call into the image and onto the device, and `b` and `r` filled but for the launch form's fields.
// `extra`: one more array of doubles that only the caller's kernel reads; *d_extra is where it lies on the device.  A run before
// this one has synchronised its stream before it returned, so the host image is free to be rewritten
inline int mol_upload(MolInput &in, hipStream_t s, int64_t F, int64_t B, const float *d_pos, const void *d_classes, int classes_int64,
                      int E, const double *thr, int carbon, int C, const int32_t *class_slot, const double *cc_edges, int n_cc, double cc_cut,
                      const double *all_edges, int n_all, double all_cut, const double *extra, size_t n_extra, const double **d_extra, MolBatch &b,
                      MolRule &r) {
    if (carbon < -1 || carbon >= E) return sm_fail(std::string(in.what) + ": the carbon slot lies outside the rule");
    const MolPlan &pl = in.plan;
    unsigned char slot[kMolMaxClasses];
    for (int k = 0; k < C; ++k) slot[k] = (unsigned char)class_slot[k];
    const int zero = 0;
    std::vector<unsigned char> &img = in.up;
    img.clear();
    const size_t o_thr = put(img, thr, (size_t)3 * E * E), o_extra = put(img, extra, n_extra);
    const size_t o_cc = put(img, cc_edges, (size_t)n_cc), o_all = put(img, all_edges, (size_t)n_all);
    const size_t o_mol = put(img, pl.mol.data(), pl.mol.size());
    in.o_wave = put(img, pl.wave.jobs.data(), pl.wave.jobs.size()); in.o_block = put(img, pl.block.jobs.data(), pl.block.jobs.size());
    const size_t o_slot = put(img, slot, (size_t)C);
    in.o_bad = put(img, &zero, 1);
    SMCHK(grow(in.mem_in, {dev_buf(&in.d_in, img.size())}, in.cap_in, (int64_t)img.size()));
    SMCHK(hipMemcpyAsync(in.d_in, img.data(), img.size(), hipMemcpyHostToDevice, s));
    const auto doubles = [&](size_t o) { return reinterpret_cast<const double *>(in.d_in + o); };
    b = MolBatch{};
    b.pos = d_pos; b.cls = d_classes; b.cls64 = classes_int64 != 0;
    b.N = pl.N; b.F = (int)F; b.B = (int)B;
    b.mol = reinterpret_cast<const MolSpan *>(in.d_in + o_mol);
    b.bad = reinterpret_cast<int *>(in.d_in + in.o_bad);
    r = MolRule{doubles(o_thr), in.d_in + o_slot, E, C, carbon, doubles(o_cc), doubles(o_all), n_cc, n_all, cc_cut, all_cut};
    *d_extra = doubles(o_extra);
    return 0;
}

// the C-C, all-pairs and class counters of a call, set to zero on the stream
inline int mol_zero_counts(MolCounts &o, int64_t *d_hist_cc, int64_t *d_hist_all, int64_t *d_class_counts, const MolBatch &b, const MolRule &r, hipStream_t s) {
    SMCHK(hipMemsetAsync(d_hist_cc, 0, (size_t)b.F * (r.n_cc + 1) * 8, s));
    SMCHK(hipMemsetAsync(d_hist_all, 0, (size_t)b.F * (r.n_all + 1) * 8, s));
    SMCHK(hipMemsetAsync(d_class_counts, 0, (size_t)b.F * r.C * 8, s));
    o = {reinterpret_cast<unsigned long long *>(d_hist_cc), reinterpret_cast<unsigned long long *>(d_hist_all), reinterpret_cast<unsigned long long *>(d_class_counts)};
    return 0;
}

// a kernel's wave and block instantiations over the job lists of the uploaded plan; Args holds the batch as `b`
template <typename Args> void mol_launch(void (*wave)(Args), void (*block)(Args), const MolInput &in, Args a, hipStream_t s) {
    const MolForm *form[2] = {&in.plan.wave, &in.plan.block};
    void (*const kernel[2])(Args) = {wave, block};
    const size_t o_jobs[2] = {in.o_wave, in.o_block};
    for (int k = 0; k < 2; ++k) {
        if (!form[k]->gx) continue;
        a.b.jobs = reinterpret_cast<const int *>(in.d_in + o_jobs[k]); a.b.n_jobs = (int)form[k]->jobs.size(); a.b.gx = form[k]->gx; a.b.iters = form[k]->iters;
        hipLaunchKernelGGL(kernel[k], dim3((unsigned)((int64_t)form[k]->gx * a.b.F)), dim3(kMolThreads), 0, s, a);
    }
}

// the end of a run: launch errors, the synchronise, and the refusal when atoms had a class outside the C classes
inline int mol_finish(const MolInput &in, int C, hipStream_t s) {
    SMCHK(hipGetLastError());
    int bad = 0;
    SMCHK(hipMemcpyAsync(&bad, in.d_in + in.o_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    SMCHK(hipStreamSynchronize(s));
    if (bad) return sm_fail(std::string(in.what) + ": " + std::to_string(bad) + " atom(s) have a class outside the " + std::to_string(C) + " classes; the outputs are not valid");
    return 0;
}

}  // namespace
