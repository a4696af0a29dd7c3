// C ABI of the molecular-surface builder (include/shapemol_hip.h, shapemol_msurf_*): closed triangle meshes of a batch of
// molecules from atom centres and radii, on the device.  The rule, the kernels and the host plan: sm_mol_surface.h.
#include "../../include/shapemol_hip.h"
#include "sm_mol_surface.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <cstring>
#include <string>
#include <vector>

namespace {
constexpr int kMsurfStages = 6;           // field, erode, count, scan, verts, faces
}  // namespace

struct shapemol_msurf_ctx {
    int device = 0;
    MsurfPlan plan;                       // of the last batch (the upload reads it until the call's synchronise)
    std::vector<unsigned char> up;        // the upload's host image: molecules, atoms, distance table
    std::vector<int> counts;
    std::vector<double> h_centres, h_radii;      // device inputs, fetched for the plan
    long long n_verts = 0, n_faces = 0;   // of the last build
    bool built = false;                   // the last build succeeded: its outputs and field can be copied
    hipEvent_t ev[kMsurfStages + 1] = {};
    // device memory: every group of buffers beside the capacity it shares (sm_devmem.h)
    unsigned char *d_in = nullptr; int64_t cap_in = 0; DevList mem_in;                                 // the upload, bytes
    double *g = nullptr; unsigned char *outside = nullptr, *emask = nullptr, *ntri = nullptr; int *vbase = nullptr;
    int64_t cap_n = 0; DevList mem_n;                                                                    // per node
    unsigned long long *chunk = nullptr; int64_t cap_c = 0; DevList mem_c;                             // per scan block
    int *d_counts = nullptr; int64_t cap_b = 0; DevList mem_b;                                         // per molecule
    double *verts = nullptr; int64_t cap_v = 0; DevList mem_v;                                         // the outputs
    int *faces = nullptr; int64_t cap_f = 0; DevList mem_f;
};

extern "C" {

int shapemol_msurf_sizes(int64_t *out, int32_t n) {
    const int64_t v[8] = {kMsurfMaxNodes, kMsurfMaxBatchNodes, kMsurfMaxAtoms, kMsurfMaxStencil, kMsurfTile, kMsurfScanBlock, kMsurfMaxMols, kMsurfScanWidth};
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return 8;
}

int shapemol_msurf_check(int64_t n_mols, const int64_t *h_atom_off, const double *h_centres, const double *h_radii, double probe_radius,
                         double spacing, double scaling) {
    const std::string e = msurf_plan(n_mols, h_atom_off, h_centres, h_radii, probe_radius, spacing, scaling, nullptr);
    return e.empty() ? 0 : sm_fail(e);
}

int shapemol_msurf_create(int device, shapemol_msurf_ctx **out) {
    if (!out) return sm_fail("shapemol_msurf_create: null argument");
    if (sm_open_device(device, "shapemol_msurf_create")) return 1;
    shapemol_msurf_ctx *c = new shapemol_msurf_ctx;
    c->device = device;
    for (hipEvent_t &e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            for (hipEvent_t &d : c->ev) if (d) (void)hipEventDestroy(d);
            delete c;
            return sm_fail("shapemol_msurf_create: hipEventCreate failed");
        }
    *out = c;
    return 0;
}

void shapemol_msurf_destroy(shapemol_msurf_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    for (hipEvent_t &e : c->ev) (void)hipEventDestroy(e);
    delete c;                              // the lists free their buffers
}

int shapemol_msurf_build(shapemol_msurf_ctx *c, int64_t n_mols, const int64_t *h_atom_off, const double *centres, const double *radii,
                         int32_t inputs_on_device, double probe_radius, double spacing, double scaling, int32_t *h_counts, double *h_lo,
                         int32_t *h_dims, double *h_stage_ms, void *stream) {
    if (!c) return sm_fail("shapemol_msurf_build: null context");
    if (!h_counts) return sm_fail("shapemol_msurf_build: h_counts is missing");
    c->n_verts = c->n_faces = 0;
    c->built = false;
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (inputs_on_device) {               // the grids are laid out on the host
        if (n_mols < 1 || n_mols > kMsurfMaxMols || !h_atom_off || !centres || !radii || h_atom_off[0] != 0 || h_atom_off[n_mols] < 1 ||
            h_atom_off[n_mols] > (int64_t)kMsurfMaxMols * kMsurfMaxAtoms)
            return sm_fail("molecular surface: bad molecule count, offsets or input pointers");
        const size_t N = (size_t)h_atom_off[n_mols];
        c->h_centres.resize(3 * N); c->h_radii.resize(N);
        SMCHK(hipMemcpyAsync(c->h_centres.data(), centres, 24 * N, hipMemcpyDeviceToHost, s));
        SMCHK(hipMemcpyAsync(c->h_radii.data(), radii, 8 * N, hipMemcpyDeviceToHost, s));
        SMCHK(hipStreamSynchronize(s));
        centres = c->h_centres.data(); radii = c->h_radii.data();
    }
    // a build before this one has synchronised its stream before it returned: the host image is free to be rewritten
    const std::string err = msurf_plan(n_mols, h_atom_off, centres, radii, probe_radius, spacing, scaling, &c->plan);
    if (!err.empty()) return sm_fail(err);
    MsurfPlan &pl = c->plan;
    const int B = (int)n_mols;
    const size_t o_mol = 0, o_atoms = (sizeof(MsurfMol) * B + 31) / 32 * 32, o_dtab = o_atoms + pl.atoms.size() * 8;
    const size_t bytes = o_dtab + pl.dtab.size() * 8;
    c->up.resize(bytes);
    std::memcpy(c->up.data() + o_atoms, pl.atoms.data(), pl.atoms.size() * 8);
    std::memcpy(c->up.data() + o_dtab, pl.dtab.data(), pl.dtab.size() * 8);
    std::memcpy(c->up.data() + o_mol, pl.mol.data(), sizeof(MsurfMol) * B);
    SMCHK(grow(c->mem_in, {dev_buf(&c->d_in, bytes)}, c->cap_in, (int64_t)bytes));
    SMCHK(grow(c->mem_n, {dev_buf(&c->g, (size_t)pl.nodes * 8), dev_buf(&c->outside, (size_t)pl.nodes), dev_buf(&c->emask, (size_t)pl.nodes),
                             dev_buf(&c->ntri, (size_t)pl.nodes), dev_buf(&c->vbase, (size_t)pl.nodes * 4)}, c->cap_n, pl.nodes));
    SMCHK(grow(c->mem_c, {dev_buf(&c->chunk, (size_t)pl.chunks * 8)}, c->cap_c, pl.chunks));
    SMCHK(grow(c->mem_b, {dev_buf(&c->d_counts, (size_t)B * 8)}, c->cap_b, B));
    SMCHK(hipMemcpyAsync(c->d_in, c->up.data(), bytes, hipMemcpyHostToDevice, s));
    MsurfArgs a{};
    a.mol = reinterpret_cast<const MsurfMol *>(c->d_in + o_mol);
    a.atoms = reinterpret_cast<const double4 *>(c->d_in + o_atoms);
    a.dtab = reinterpret_cast<const double *>(c->d_in + o_dtab);
    a.g = c->g; a.outside = c->outside; a.emask = c->emask; a.ntri = c->ntri; a.vbase = c->vbase; a.chunk = c->chunk; a.counts = c->d_counts;
    a.h = pl.h; a.p = pl.p; a.R = pl.R;
    const bool timed = h_stage_ms != nullptr;
    int stage = 0;
    auto mark = [&]() { return timed ? hipEventRecord(c->ev[stage++], s) : hipSuccess; };
    SMCHK(mark());
    hipLaunchKernelGGL(msurf_field_kernel, dim3((unsigned)((pl.max_nodes + 255) / 256), (unsigned)B), dim3(256), 0, s, a);
    SMCHK(mark());
    if (pl.R > 0) {
        const int W = kMsurfTile + 2 * pl.R;
        hipLaunchKernelGGL(msurf_erode_kernel, dim3((unsigned)pl.max_tiles, (unsigned)B), dim3(512), (size_t)W * W * W, s, a);
    }
    SMCHK(mark());
    hipLaunchKernelGGL(msurf_count_kernel, dim3((unsigned)pl.max_chunks, (unsigned)B), dim3(256), 0, s, a);
    SMCHK(mark());
    hipLaunchKernelGGL(msurf_scan_kernel, dim3((unsigned)B), dim3(kMsurfScanWidth), 0, s, a);
    SMCHK(hipGetLastError());
    c->counts.resize(2 * (size_t)B);
    SMCHK(hipMemcpyAsync(c->counts.data(), c->d_counts, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    SMCHK(hipStreamSynchronize(s));
    long long nv = 0, nf = 0;
    for (int b = 0; b < B; ++b) {
        pl.mol[b].vert_off = nv; pl.mol[b].face_off = nf;
        nv += c->counts[2 * b]; nf += c->counts[2 * b + 1];
        h_counts[2 * b] = c->counts[2 * b]; h_counts[2 * b + 1] = c->counts[2 * b + 1];
        for (int k = 0; k < 3; ++k) {
            if (h_lo) h_lo[3 * b + k] = pl.mol[b].lo[k];
            if (h_dims) h_dims[3 * b + k] = pl.mol[b].n[k];
        }
    }
    SMCHK(grow(c->mem_v, {dev_buf(&c->verts, (size_t)std::max(nv, 1ll) * 24)}, c->cap_v, std::max(nv, 1ll)));
    SMCHK(grow(c->mem_f, {dev_buf(&c->faces, (size_t)std::max(nf, 1ll) * 12)}, c->cap_f, std::max(nf, 1ll)));
    a.verts = c->verts; a.faces = c->faces;
    std::memcpy(c->up.data() + o_mol, pl.mol.data(), sizeof(MsurfMol) * B);      // now with the output offsets
    SMCHK(hipMemcpyAsync(c->d_in + o_mol, c->up.data() + o_mol, sizeof(MsurfMol) * B, hipMemcpyHostToDevice, s));
    SMCHK(mark());
    hipLaunchKernelGGL(msurf_verts_kernel, dim3((unsigned)pl.max_chunks, (unsigned)B), dim3(256), 0, s, a);
    SMCHK(mark());
    hipLaunchKernelGGL(msurf_faces_kernel, dim3((unsigned)pl.max_chunks, (unsigned)B), dim3(256), 0, s, a);
    SMCHK(mark());
    SMCHK(hipGetLastError());
    SMCHK(hipStreamSynchronize(s));
    if (timed)
        for (int i = 0; i < kMsurfStages; ++i) {
            float ms = 0;
            SMCHK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
            h_stage_ms[i] = ms;
        }
    c->n_verts = nv; c->n_faces = nf;
    c->built = true;
    return 0;
}

int shapemol_msurf_copy(shapemol_msurf_ctx *c, int32_t which, void *dst, int64_t n_items, void *stream) {
    if (!c || !dst) return sm_fail("shapemol_msurf_copy: null argument");
    const void *src = which == 0 ? (const void *)c->verts : which == 1 ? (const void *)c->faces : which == 2 ? (const void *)c->g : nullptr;
    const long long have = which == 0 ? c->n_verts * 3 : which == 1 ? c->n_faces * 3 : c->plan.nodes;
    const size_t size = which == 1 ? 4 : 8;
    if (!c->built || !src || n_items < 0 || n_items > have) return sm_fail("shapemol_msurf_copy: nothing of that kind and size from the last build");
    SMCHK(hipSetDevice(c->device));
    if (n_items) SMCHK(hipMemcpyAsync(dst, src, (size_t)n_items * size, hipMemcpyDefault, (hipStream_t)stream));
    SMCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
