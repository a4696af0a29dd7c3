// C ABI of the bond graphs of sampled molecules (include/shapemol_hip.h, shapemol_graph_*): bonds with orders, fragments,
// completeness, rings and bond-length histograms for every frame of a packed batch, on the device.  The kernels: sm_mol_graph.h;
// the arithmetic and the host plan: sm_mol_rule.h; the upload and the launch: sm_mol_upload.h.
#include "../../include/shapemol_hip.h"
#include "sm_mol_graph.h"
#include "sm_mol_upload.h"

struct shapemol_graph_ctx {
    int device = 0;
    MolInput in{"bond graph"};            // the plan and the upload
    int *d_count = nullptr; long long *d_offset = nullptr; int64_t cap_fb = 0; DevList mem_fb;       // per (frame, molecule)
    int *d_bonds = nullptr, *d_ring = nullptr; int64_t cap_b = 0; DevList mem_b;                     // per bond
    int64_t n_fb = 0, total = -1;         // of the last run that reached its fill pass; total < 0: none
};

extern "C" {

int shapemol_graph_sizes(int64_t *out, int32_t n) {
    const int64_t v[7] = {kMolWaveAtoms, kMgraphMaxAtoms, kMolMaxElements, kMolMaxClasses, kMolMaxEdges, kMolThreads, kMgraphRingBits};
    for (int i = 0; i < n && i < 7; ++i) out[i] = v[i];
    return 7;
}

int shapemol_graph_check(int64_t n_frames, int64_t n_mols, const int64_t *h_off, int32_t n_elements, int32_t n_classes, const int32_t *h_class_slot,
                         const double *h_cc_edges, int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all, double all_cut,
                         const double *h_bl_edges, int32_t n_bl, int32_t *h_forms) {
    MolPlan pl;
    const std::string e = mgraph_plan(n_frames, n_mols, h_off, n_elements, n_classes, h_class_slot, h_cc_edges, n_cc, cc_cut, h_all_edges, n_all, all_cut,
                                      h_bl_edges, n_bl, &pl);
    if (!e.empty()) return sm_fail(e);
    if (h_forms) std::memcpy(h_forms, pl.form.data(), pl.form.size() * sizeof(int));
    return 0;
}

int shapemol_graph_create(int device, shapemol_graph_ctx **out) {
    if (!out) return sm_fail("shapemol_graph_create: null argument");
    if (sm_open_device(device, "shapemol_graph_create")) return 1;
    shapemol_graph_ctx *c = new shapemol_graph_ctx;
    c->device = device;
    *out = c;
    return 0;
}

void shapemol_graph_destroy(shapemol_graph_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                              // the lists free their buffers
}

int shapemol_graph_run(shapemol_graph_ctx *c, int64_t n_frames, int64_t n_mols, const int64_t *h_off, const float *d_pos, const void *d_classes,
                       int32_t classes_int64, int32_t n_elements, const double *h_thresholds, int32_t carbon_slot, int32_t n_classes,
                       const int32_t *h_class_slot, const double *h_cc_edges, int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all,
                       double all_cut, const double *h_bl_edges, int32_t n_bl, int32_t *d_nr_bonds, int32_t *d_degree, int32_t *d_frag,
                       int32_t *d_ring_atom, int32_t *d_mol, int64_t *d_hist_bl, int64_t *d_hist_cc, int64_t *d_hist_all, int64_t *d_class_counts,
                       int64_t *d_frame_counts, int64_t *h_total, void *stream) {
    if (!c) return sm_fail("shapemol_graph_run: null context");
    if (!d_pos || !d_classes || !h_thresholds || !d_nr_bonds || !d_degree || !d_frag || !d_ring_atom || !d_mol || !d_hist_bl || !d_hist_cc || !d_hist_all ||
        !d_class_counts || !d_frame_counts || !h_total)
        return sm_fail("shapemol_graph_run: null argument");
    const std::string err = mgraph_plan(n_frames, n_mols, h_off, n_elements, n_classes, h_class_slot, h_cc_edges, n_cc, cc_cut, h_all_edges, n_all, all_cut,
                                        h_bl_edges, n_bl, &c->in.plan);
    if (!err.empty()) return sm_fail(err);
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_fb = n_frames * n_mols;
    c->total = -1;
    MgraphArgs a{};
    if (mol_upload(c->in, s, n_frames, n_mols, d_pos, d_classes, classes_int64, n_elements, h_thresholds, carbon_slot, n_classes, h_class_slot, h_cc_edges,
                   n_cc, cc_cut, h_all_edges, n_all, all_cut, h_bl_edges, (size_t)n_bl, &a.bl_edges, a.b, a.r))
        return 1;
    SMCHK(grow(c->mem_fb, {dev_buf(&c->d_count, (size_t)n_fb * sizeof(int)), dev_buf(&c->d_offset, (size_t)(n_fb + 1) * sizeof(long long))}, c->cap_fb, n_fb));
    a.n_bl = n_bl;
    a.count = c->d_count; a.offset = c->d_offset;
    // count, scan, and the one synchronisation that tells the host how many bonds there are
    mol_launch(mgraph_kernel<64, 0>, mgraph_kernel<kMolThreads, 0>, c->in, a, s);
    hipLaunchKernelGGL(mgraph_scan_kernel, dim3(1), dim3(kMolThreads), 0, s, c->d_count, c->d_offset, (long long)n_fb);
    SMCHK(hipGetLastError());
    long long total = 0;
    SMCHK(hipMemcpyAsync(&total, c->d_offset + n_fb, sizeof(long long), hipMemcpyDeviceToHost, s));
    SMCHK(hipStreamSynchronize(s));
    if (total < 0 || total >= (1ll << 31)) return sm_fail("bond graph: " + std::to_string(total) + " bonds in this call; the limit is 2^31 - 1 (pass fewer frames)");
    const int64_t need_b = std::max<int64_t>(total, 1);
    SMCHK(grow(c->mem_b, {dev_buf(&c->d_bonds, (size_t)3 * need_b * sizeof(int)), dev_buf(&c->d_ring, (size_t)need_b * sizeof(int))}, c->cap_b, need_b));
    const size_t np = (size_t)n_elements * (n_elements + 1) / 2;
    SMCHK(hipMemsetAsync(d_hist_bl, 0, (size_t)n_frames * 2 * np * 3 * (n_bl + 1) * 8, s));
    SMCHK(hipMemsetAsync(d_frame_counts, 0, (size_t)n_frames * (1 + kMgraphRingBits) * 8, s));
    if (mol_zero_counts(a.o, d_hist_cc, d_hist_all, d_class_counts, a.b, a.r, s)) return 1;
    a.nr_bonds = d_nr_bonds; a.degree = d_degree; a.frag = d_frag; a.ring_atom = d_ring_atom; a.mol_out = d_mol;
    a.bonds = c->d_bonds; a.ring_bond = c->d_ring;
    a.hist_bl = reinterpret_cast<unsigned long long *>(d_hist_bl);
    a.frame_counts = reinterpret_cast<unsigned long long *>(d_frame_counts);
    mol_launch(mgraph_kernel<64, 1>, mgraph_kernel<kMolThreads, 1>, c->in, a, s);
    if (mol_finish(c->in, n_classes, s)) return 1;
    c->n_fb = n_fb; c->total = total;
    *h_total = total;
    return 0;
}

int shapemol_graph_bonds(shapemol_graph_ctx *c, int32_t which, void *dst, int64_t n_items, void *stream) {
    if (!c || !dst) return sm_fail("shapemol_graph_bonds: null argument");
    const void *src = which == 0 ? (const void *)c->d_offset : which == 1 ? (const void *)c->d_bonds : which == 2 ? (const void *)c->d_ring : nullptr;
    const int64_t have = which == 0 ? c->n_fb + 1 : which == 1 ? 3 * c->total : c->total;
    const size_t size = which == 0 ? 8 : 4;
    if (c->total < 0 || !src || n_items < 0 || n_items > have) return sm_fail("shapemol_graph_bonds: nothing of that kind and size from the last run");
    SMCHK(hipSetDevice(c->device));
    if (n_items) SMCHK(hipMemcpyAsync(dst, src, (size_t)n_items * size, hipMemcpyDefault, (hipStream_t)stream));
    SMCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int shapemol_graph_debug_fill(shapemol_graph_ctx *c, int32_t byte, void *stream) {
    if (!c) return sm_fail("shapemol_graph_debug_fill: null context");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (c->in.cap_in) SMCHK(hipMemsetAsync(c->in.d_in, byte, (size_t)c->in.cap_in, s));
    if (c->cap_fb) {
        SMCHK(hipMemsetAsync(c->d_count, byte, (size_t)c->cap_fb * sizeof(int), s));
        SMCHK(hipMemsetAsync(c->d_offset, byte, (size_t)(c->cap_fb + 1) * sizeof(long long), s));
    }
    if (c->cap_b) {
        SMCHK(hipMemsetAsync(c->d_bonds, byte, (size_t)3 * c->cap_b * sizeof(int), s));
        SMCHK(hipMemsetAsync(c->d_ring, byte, (size_t)c->cap_b * sizeof(int), s));
    }
    SMCHK(hipStreamSynchronize(s));
    c->total = -1;                         // nothing of the last run is left to copy
    return 0;
}

}  // extern "C"
