// C ABI of the shape auto-encoder's batch builder (include/shapemol_hip.h, shapemol_sdata_*): surface clouds, query points and
// their signed distances / occupancies for a batch of triangle meshes, on the device.  Kernels and the host image: sm_shape_data.h.
#include "../../include/shapemol_hip.h"
#include "sm_shape_data.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <string>
#include <vector>

struct shapemol_sdata_ctx {
    int device = 0;
    SdataImage im;                        // what the host uploaded for the last batch (the upload reads it until the call's synchronise)
    // device memory: every group of buffers beside the capacity it shares (sm_devmem.h).  A build rewrites all of it: one
    // stream at a time
    unsigned char *d_in = nullptr; int64_t cap_in = 0; DevList mem_in;                           // the upload, bytes
    MeshFace *faces = nullptr; double4 *fbox = nullptr; int64_t cap_f = 0; DevList mem_f;        // the face image, F faces
    float *cloud32 = nullptr; int64_t cap_p = 0; DevList mem_p;                                  // B x P points
    double *cand = nullptr, *dist = nullptr; int *flag = nullptr; int64_t cap_q = 0; DevList mem_q;   // B x 3T candidates
    int *counts = nullptr; int64_t cap_b = 0; DevList mem_b;                                     // B shapes
};

extern "C" {

int shapemol_sdata_check(int64_t n_shapes, const int64_t *h_vert_off, const double *h_verts, const int64_t *h_face_off, const int32_t *h_faces,
                         int64_t n_cloud, int64_t n_samples, int32_t loss_type) {
    const std::string e = sdata_check(n_shapes, h_vert_off, h_verts, h_face_off, h_faces, n_cloud, n_samples, loss_type);
    return e.empty() ? 0 : sm_fail(e);
}

int shapemol_sdata_create(int device, shapemol_sdata_ctx **out) {
    if (!out) return sm_fail("shapemol_sdata_create: null argument");
    if (sm_open_device(device, "shapemol_sdata_create")) return 1;
    shapemol_sdata_ctx *c = new shapemol_sdata_ctx;
    c->device = device;
    *out = c;
    return 0;
}

void shapemol_sdata_destroy(shapemol_sdata_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                              // the lists free their buffers
}

int shapemol_sdata_build(shapemol_sdata_ctx *c, int64_t n_shapes, const int64_t *h_vert_off, const double *h_verts, const int64_t *h_face_off,
                         const int32_t *h_faces, int64_t n_cloud, int64_t n_samples, int32_t loss_type, const double *d_cloud_draws,
                         const double *d_query_draws, uint64_t seed, float *d_cloud, float *d_points, float *d_values, float *d_centres,
                         float *d_bounds, int32_t *h_counts, int32_t *d_face_idx, int32_t *d_flags, int32_t *d_sel, void *stream) {
    if (!c) return sm_fail("shapemol_sdata_build: null context");
    if (shapemol_sdata_check(n_shapes, h_vert_off, h_verts, h_face_off, h_faces, n_cloud, n_samples, loss_type)) return 1;
    if (!d_cloud || !d_centres || !d_bounds || (n_samples > 0 && (!d_points || !d_values || !h_counts)))
        return sm_fail("shapemol_sdata_build: an output pointer is missing");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int B = (int)n_shapes, P = (int)n_cloud, T = (int)n_samples;
    const int64_t Q = 3 * (int64_t)T;
    // a build before this one has synchronised its stream before it returned: the host image is free to be rewritten
    sdata_image(B, h_vert_off, h_verts, h_face_off, h_faces, c->im);
    const int64_t bytes = (int64_t)c->im.bytes.size();
    SMCHK(grow(c->mem_in, {dev_buf(&c->d_in, (size_t)bytes)}, c->cap_in, bytes));
    SMCHK(grow(c->mem_p, {dev_buf(&c->cloud32, (size_t)B * P * 12)}, c->cap_p, (int64_t)B * P));
    if (T > 0) {
        SMCHK(grow(c->mem_f, {dev_buf(&c->faces, (size_t)c->im.F * sizeof(MeshFace)), dev_buf(&c->fbox, (size_t)c->im.F * sizeof(double4))}, c->cap_f, c->im.F));
        SMCHK(grow(c->mem_q, {dev_buf(&c->cand, (size_t)B * Q * 24), dev_buf(&c->dist, (size_t)B * Q * 8), dev_buf(&c->flag, (size_t)B * Q * 4)},
                      c->cap_q, (int64_t)B * Q));
    }
    SMCHK(grow(c->mem_b, {dev_buf(&c->counts, (size_t)B * 8)}, c->cap_b, (int64_t)B));
    SMCHK(hipMemcpyAsync(c->d_in, c->im.bytes.data(), (size_t)bytes, hipMemcpyHostToDevice, s));
    SdataArgs a{};
    const SdataImage &im = c->im;
    a.verts = reinterpret_cast<const double *>(c->d_in + im.o_verts); a.face_ix = reinterpret_cast<const int *>(c->d_in + im.o_ix);
    a.cdf = reinterpret_cast<const double *>(c->d_in + im.o_cdf); a.vert_off = reinterpret_cast<const int *>(c->d_in + im.o_voff);
    a.faces = c->faces; a.fbox = c->fbox;
    a.pbounds = reinterpret_cast<const double *>(c->d_in + im.o_pb); a.lohi = reinterpret_cast<const double *>(c->d_in + im.o_lohi);
    a.face_off = reinterpret_cast<const int *>(c->d_in + im.o_off);
    a.cloud_draws = d_cloud_draws; a.query_draws = d_query_draws; a.seed = seed;
    a.cloud32 = c->cloud32; a.cand = c->cand; a.dist = c->dist; a.flag = c->flag; a.counts = c->counts;
    a.cloud_out = d_cloud; a.points = d_points; a.values = d_values; a.centres = d_centres; a.bounds = d_bounds;
    a.face_idx = d_face_idx; a.flag_out = d_flags; a.sel = d_sel;
    a.B = B; a.P = P; a.T = T; a.occupancy = loss_type == SHAPEMOL_SD_OCCUPANCY;
    hipLaunchKernelGGL(sdata_cloud_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0, s, a);
    if (T > 0) {
        hipLaunchKernelGGL(sdata_image_kernel, dim3((unsigned)((im.max_faces + 255) / 256), (unsigned)B), dim3(256), 0, s, a);
        hipLaunchKernelGGL(sdata_classify_kernel, dim3((unsigned)((Q + 15) / 16), (unsigned)B), dim3(256), mesh_lds_bytes(P), s, a);
    }
    hipLaunchKernelGGL(sdata_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
    SMCHK(hipGetLastError());
    if (T > 0) SMCHK(hipMemcpyAsync(h_counts, c->counts, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    SMCHK(hipStreamSynchronize(s));
    if (T > 0) {
        std::string shy;
        for (int b = 0; b < B; ++b) {
            const int n_in = std::min(T / 2, (int)h_counts[2 * b]);
            if (h_counts[2 * b + 1] < T - n_in)
                shy += (shy.empty() ? "" : ", ") + std::to_string(b) + " (" + std::to_string(h_counts[2 * b]) + " inside, " + std::to_string(h_counts[2 * b + 1]) +
                       " outside of " + std::to_string(Q) + " candidates; " + std::to_string(T - n_in) + " outside rows needed)";
        }
        if (!shy.empty()) {
            sm_fail("shape data: too few candidates outside the mesh to fill num_samples rows (the reference's torch.stack fails there) for shape " + shy);
            return 2;
        }
    }
    return 0;
}

}  // extern "C"
