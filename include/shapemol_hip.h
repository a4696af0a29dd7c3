/*
 * shapemol_hip.h -- C ABI of the MI355X (gfx950) implementation of ShapeMol's denoising hot path.
 *
 * The reference has no FFI of its own (it is pure Python on third-party torch ops), so the
 * boundary is its Python call surface; each entry point below names the reference call it
 * replaces (paths relative to the reference repository root):
 *
 *   shapemol_create / _destroy     ScorePosNet3D.__init__ + load_state_dict
 *                                  models/molopt_score_model.py:171-283, scripts/sample_diffusion.py:211-215
 *   shapemol_score                 ScorePosNet3D.forward        models/molopt_score_model.py:286-320
 *                                  (-> UniTransformerO2TwoUpdateGeneral.forward, models/uni_transformer.py:483-540)
 *   shapemol_sample                ScorePosNet3D.sample_diffusion  models/molopt_score_model.py:533-697
 *   shapemol_log_sample_categorical  log_sample_categorical     models/molopt_score_model.py:98-104
 *
 * Conventions
 *   - plain pointers and sizes only; every `d_` pointer is DEVICE memory on the context's device,
 *     caller-owned, float32 / int64 exactly as the reference's tensors (row-major, contiguous);
 *     outputs are caller-allocated.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - no hidden host synchronisation in _score/_sample/_log_sample_categorical: work is enqueued on
 *     `stream` and the call returns; the caller synchronises.
 *   - return 0 on success, non-zero on error; shapemol_last_error() returns the message of the last
 *     failing call on this thread.
 *   - one context per device; a context is not thread-safe.
 */
#ifndef SHAPEMOL_HIP_H
#define SHAPEMOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHAPEMOL_ABI_VERSION 5

typedef struct shapemol_ctx shapemol_ctx;

/* `model` section of the training YAML (the YAML files under config/training, lines 21-74), reduced to what the path uses. */
typedef struct shapemol_config {
    int32_t hidden_dim;        /* 128 */
    int32_t n_heads;           /* 16  (hidden_dim / n_heads must be 8) */
    int32_t num_layers;        /* 8   */
    int32_t knn;               /* 8   (1..32) */
    int32_t num_r_gaussian;    /* 20  (the reference hard-codes 20 centres) */
    int32_t shape_dim;         /* 32  point-cloud latent vectors per molecule, each in R^3 */
    int32_t shape_latent_dim;  /* 32  */
    int32_t time_emb_dim;      /* 8   */
    int32_t num_classes;       /* 15  */
    int32_t num_timesteps;     /* 1000 */
} shapemol_config;

int shapemol_abi_version(void);
const char *shapemol_last_error(void);

/* Number of float32 values shapemol_create expects in `weights` for this config: every float entry
 * of the reference state dict, in registration order, densely concatenated (the int64
 * `num_batches_tracked` counters are skipped).  shapemol_amd.pack_state_dict builds it. */
size_t shapemol_weight_count(const shapemol_config *cfg);

/* weights: HOST pointer to shapemol_weight_count() floats.  device: HIP device ordinal. */
int shapemol_create(const shapemol_config *cfg, const float *weights, size_t n_weights,
                    int device, shapemol_ctx **out);
void shapemol_destroy(shapemol_ctx *ctx);

/* Pre-size the workspace (otherwise it grows on demand, which allocates). */
int shapemol_reserve(shapemol_ctx *ctx, int64_t max_atoms, int64_t max_mols);

/* One score evaluation.
 *   d_pos   (N,3) f32   ligand_pos_perturbed      d_v     (N,) i64  ligand_v_perturbed
 *   d_batch (N,) i64 sorted molecule id per atom  d_shape (B,shape_dim,3) f32  ligand_shape
 *   d_t     (B,) i64    time_step
 *   out_pos (N,3) f32   pred_ligand_pos   out_h (N,H) f32 pred_ligand_h (may be NULL)
 *   out_v   (N,C) f32   pred_ligand_v */
int shapemol_score(shapemol_ctx *ctx, const float *d_pos, const int64_t *d_v, const int64_t *d_batch,
                   int64_t n_atoms, int64_t n_mols, const float *d_shape, const int64_t *d_t,
                   float *out_pos, float *out_h, float *out_v, void *stream);

/* Trajectory buffers of shapemol_sample; any pointer may be NULL (that trajectory is not kept).
 * All are DEVICE buffers with a leading num_steps dimension. */
typedef struct shapemol_traj {
    float   *pos_traj;       /* (S,N,3)  x_{t-1} after each step          (pos_traj)       */
    int64_t *v_traj;         /* (S,N)    v_{t-1} after each step          (v_traj)         */
    float   *v0_traj;        /* (S,N,C)  log_softmax of predicted logits  (v0_traj)        */
    float   *vt_traj;        /* (S,N,C)  log posterior q(v_{t-1}|v_t,v0)  (vt_traj)        */
    float   *pos_cond_traj;  /* (S,N,3)  raw network x0 prediction        (pos_cond_traj)  */
    float   *v_cond_traj;    /* (S,N,C)  raw network logits               (v_cond_traj)    */
} shapemol_traj;

/* Reverse chain t = T-1 ... T-num_steps (center_pos_mode 'none', no guidance).
 *   d_init_pos (N,3) f32, d_init_v (N,) i64, d_batch, d_shape as in shapemol_score.
 *   Noise: if d_eps != NULL and d_u != NULL they are host-chosen draws, eps (S,N,3) ~ N(0,1) and
 *   u (S,N,C) ~ U[0,1), consumed per step in the reference's order (randn_like then rand_like,
 *   models/molopt_score_model.py:662,99).  Otherwise noise is generated on the device
 *   (Philox4x32-10 keyed by `seed`, Box-Muller).
 *   out_pos (N,3) f32, out_v (N,) i64: final state.  use_graph != 0 replays a captured hipGraph of one
 *   reverse step (and of twenty steps back to back).  The capture depends on (n_atoms, n_mols) only: seed,
 *   noise and trajectory pointers are passed through device memory, so chains with new seeds or new result
 *   buffers replay the same executable. */
int shapemol_sample(shapemol_ctx *ctx, const float *d_init_pos, const int64_t *d_init_v,
                    const int64_t *d_batch, int64_t n_atoms, int64_t n_mols, const float *d_shape,
                    int32_t num_steps, const float *d_eps, const float *d_u, uint64_t seed,
                    const shapemol_traj *traj, float *out_pos, int64_t *out_v,
                    int32_t use_graph, void *stream);

/* Point-cloud shape guidance of the following _sample calls (pointcloud_shape_guidance,
 * models/molopt_score_model.py:699-740; applied to the predicted x0 of every step with t > grad_step, :583-586):
 * an atom whose three nearest cloud points are on average farther than `radius` is pulled towards their mean by a random
 * fraction in [0.2, 0.8), up to five times.  h_cloud: HOST (n_points,3) float64 (copied); n_points = 0 switches it off.
 * d_draws: DEVICE (S,5,N) float64 uniforms, the np.random.random() draw of every (step, iteration, atom) (parity mode;
 * entries of atoms that are not pulled are ignored), or NULL: Philox(seed of the chain).  Replaces the reference's
 * per-step D2H + KD-tree + H2D round trip by one kernel inside the step graph.
 * A context holds ONE set of cloud groups (shapemol_set_guidance_groups): this call installs a set of one group that spans
 * whatever batch the following _sample calls bring (no n_mols requirement), in place of the set installed before, and
 * n_points = 0 empties the slot -- also when the set in it came from shapemol_set_guidance_groups. */
int shapemol_set_guidance(shapemol_ctx *ctx, const double *h_cloud, int64_t n_points, double radius,
                          int32_t grad_step, const double *d_draws);

/* pointcloud_shape_guidance on its own (models/molopt_score_model.py:699-740): guide d_pos (N,3) f32 in place against the
 * cloud of shapemol_set_guidance (shapemol_guide_points_groups without a batch vector: the one group is all N atoms);
 * d_draws DEVICE (5,N) float64 or NULL (Philox(seed)). */
int shapemol_guide_points(shapemol_ctx *ctx, float *d_pos, int64_t n_points, const double *d_draws, uint64_t seed, void *stream);

/* Point-cloud shape guidance with one cloud per GROUP of molecules, for the following _sample calls.  Group g is the contiguous
 * run of molecules h_mol_off[g] .. h_mol_off[g + 1] - 1 of the batch (so a contiguous run of atoms); its cloud is rows
 * h_cloud_off[g] .. h_cloud_off[g + 1] - 1 of h_clouds (HOST (sum P_g, 3) float64, copied) and its radius h_radius[g].  A group
 * with an empty cloud is left unguided.  Per atom the arithmetic is shapemol_set_guidance's; d_draws is the same DEVICE
 * (S,5,N) float64 table indexed by the batch-global atom, or NULL: Philox(seed of the chain) keyed by the batch-global atom.
 * Validated on the host (offsets start at 0 and do not decrease, every non-empty cloud has 3 .. 2048 points and a radius > 0);
 * the error names the offending group.  shapemol_sample then requires n_mols == h_mol_off[n_groups].  n_groups = 0 removes the
 * groups.  The set replaces whatever shapemol_set_guidance or this function installed before; a mesh, when set, takes
 * precedence. */
int shapemol_set_guidance_groups(shapemol_ctx *ctx, int32_t n_groups, const int64_t *h_mol_off, const double *h_clouds,
                                 const int64_t *h_cloud_off, const double *h_radius, int32_t grad_step, const double *d_draws);

/* One guidance pass on its own against the groups of shapemol_set_guidance_groups: guide d_pos (n_atoms,3) f32 DEVICE in place;
 * d_batch DEVICE (n_atoms) int64, sorted, gives every atom's molecule; d_draws DEVICE (5,n_atoms) float64 or NULL (Philox(seed)). */
int shapemol_guide_points_groups(shapemol_ctx *ctx, float *d_pos, const int64_t *d_batch, int64_t n_atoms, const double *d_draws,
                                 uint64_t seed, void *stream);

/* The same as the reference's MODULE-level function pointcloud_shape_guidance(use_pointcloud_data, pred_ligand_pos, k=3,
 * ratio=0.2) (models/molopt_score_model.py:699-740), which has no model object at hand: no context, the cloud comes with
 * the call (h_cloud: HOST (n_cloud,3) float64, 3 .. 2048 points) on the CURRENT device; d_pos (n_atoms,3) f32 DEVICE is
 * guided in place; `ratio` is the lower end of the pull fraction u * (0.8 - ratio) + ratio; d_draws / seed as above.
 * Unlike the other entry points this one synchronises `stream` before it returns (it owns a temporary device block); the
 * reference's function is synchronous as well (D2H copy, host KD-tree, H2D copy). */
int shapemol_pointcloud_guidance(const double *h_cloud, int64_t n_cloud, double radius, double ratio, float *d_pos,
                                 int64_t n_atoms, const double *d_draws, uint64_t seed, void *stream);

/* Mesh shape guidance of the following _sample calls (mesh_shape_guidance, models/molopt_score_model.py:742-775; applied to the
 * predicted x0 of every step with t > grad_step, :571-580; takes precedence over the point cloud of shapemol_set_guidance).
 * The "within" atoms (inside the mesh, > 0.4 from the nearest cloud point) of the whole batch anchor the pull; every "outmesh"
 * atom (outside the mesh, or < 0.2 from the cloud) moves away from the mean of its 3 nearest within-atoms by u * 0.8 + 0.2 and
 * is accepted once inside the mesh and > 0.2 from the cloud, up to five times; atoms never accepted keep their position.
 * h_verts: HOST (n_verts,3) float64; h_faces: HOST (n_faces,3) int32 vertex indices of a closed, consistently oriented
 * triangle mesh (checked: every index in [0, n_verts), no repeated index within a face); containment is the parity of a fixed
 * ray (sm_mesh.h), not trimesh's code.  h_cloud: HOST (n_cloud,3) float64, 3 .. 2048 points.  All three are copied;
 * n_faces = 0 switches guidance off.  d_draws: DEVICE (S,5,N) float64 uniforms as for shapemol_set_guidance, or NULL
 * (Philox(seed of the chain), a counter domain of its own).  Fewer than 3 within-atoms (none at all, or fewer than 3 while
 * some atom is to be pulled) raises status flag 6 (the reference's KD-tree raises ValueError there); the step is left unguided.
 * A context holds ONE set of mesh groups (shapemol_set_mesh_guidance_groups): this call installs a set of one group that
 * spans whatever batch the following _sample calls bring (no n_mols requirement), in place of the set installed before, and
 * n_faces = 0 empties the slot -- also when the set in it came from shapemol_set_mesh_guidance_groups. */
int shapemol_set_mesh_guidance(shapemol_ctx *ctx, const double *h_verts, int64_t n_verts, const int32_t *h_faces,
                               int64_t n_faces, const double *h_cloud, int64_t n_cloud, int32_t grad_step, const double *d_draws);

/* mesh_shape_guidance on its own: guide d_pos (N,3) f32 DEVICE in place against the mesh of shapemol_set_mesh_guidance
 * (shapemol_guide_points_mesh_groups without a batch vector: the one group is all N atoms);
 * d_draws DEVICE (5,N) float64 or NULL (Philox(seed)).  Asynchronous on `stream`; the status flag as above (clear before). */
int shapemol_guide_points_mesh(shapemol_ctx *ctx, float *d_pos, int64_t n_atoms, const double *d_draws, uint64_t seed,
                               void *stream);

/* Mesh shape guidance with one mesh per GROUP of molecules, for the following _sample calls.  Group g is the contiguous run of
 * molecules h_mol_off[g] .. h_mol_off[g + 1] - 1 of the batch (so a contiguous run of atoms); its mesh is vertices
 * h_vert_off[g] .. h_vert_off[g + 1] - 1 of h_verts (HOST (sum V_g, 3) float64) and faces h_face_off[g] .. h_face_off[g + 1] - 1
 * of h_faces (HOST (sum F_g, 3) int32, indices RELATIVE to the group's first vertex), its cloud rows h_cloud_off[g] ..
 * h_cloud_off[g + 1] - 1 of h_clouds (HOST (sum P_g, 3) float64); all are copied.  One guided step is shapemol_set_mesh_guidance's
 * step applied once per group to the group's atoms: the within-atoms and the 3-nearest search among them are PER GROUP.  A
 * group with no vertices, faces and cloud is left unguided.  d_draws is the same DEVICE (S,5,N) float64 table indexed by the
 * batch-global atom, or NULL: Philox(seed of the chain) keyed by the batch-global atom (a counter domain of its own).
 * Validated on the host (all offsets start at 0 and do not decrease; every non-empty group has >= 3 vertices, >= 1 face with
 * indices inside the group's vertices and none repeated, and a cloud of 3 .. 2048 points); the error names the offending
 * group.  shapemol_sample then requires n_mols == h_mol_off[n_groups].  n_groups = 0 removes the groups.  The set replaces
 * whatever shapemol_set_mesh_guidance or this function installed before; a mesh set takes precedence over point clouds.  A
 * group with fewer than 3 within-atoms (none at all, or fewer than 3 while one of its atoms is to be pulled) raises status
 * flag 6 and is left unguided in that step; the other groups are guided (shapemol_debug_read "mesh_group_flags" tells which). */
int shapemol_set_mesh_guidance_groups(shapemol_ctx *ctx, int32_t n_groups, const int64_t *h_mol_off, const double *h_verts,
                                      const int64_t *h_vert_off, const int32_t *h_faces, const int64_t *h_face_off,
                                      const double *h_clouds, const int64_t *h_cloud_off, int32_t grad_step, const double *d_draws);

/* One guidance pass on its own against the groups of shapemol_set_mesh_guidance_groups: guide d_pos (n_atoms,3) f32 DEVICE in
 * place; d_batch DEVICE (n_atoms) int64, sorted, gives every atom's molecule; d_draws DEVICE (5,n_atoms) float64 or NULL
 * (Philox(seed)).  Asynchronous on `stream`; the status flag as above (cleared before). */
int shapemol_guide_points_mesh_groups(shapemol_ctx *ctx, float *d_pos, const int64_t *d_batch, int64_t n_atoms,
                                      const double *d_draws, uint64_t seed, void *stream);

/* The reference's MODULE-level function mesh_shape_guidance(use_mesh_data, pred_ligand_pos) without a context: mesh and cloud
 * come with the call (as for shapemol_set_mesh_guidance) on the CURRENT device, d_pos (n_atoms,3) f32 DEVICE is guided in
 * place; d_draws / seed as above.  Synchronises `stream` before it returns, like shapemol_pointcloud_guidance.  Fewer than 3
 * within-atoms: returns non-zero and sets *flag_out (may be NULL) to 1, the positions untouched. */
int shapemol_mesh_guidance(const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces,
                           const double *h_cloud, int64_t n_cloud, float *d_pos, int64_t n_atoms, const double *d_draws,
                           uint64_t seed, int32_t *flag_out, void *stream);

/* Classifier-free guidance of the following _sample calls (models/molopt_score_model.py:616-642).  Every step then evaluates
 * the score with the shape and with a zeroed shape (same positions, kNN graph and edge weights), combines the predictions as
 * (1 + guide_stren) * cond - guide_stren * uncond and applies threshold_CFG (:136-151) to positions and logits:
 * threshold_type 0 none, 1 reference_threshold (s = max|cond| * p), 2 dynamic_threshold (s = torch.quantile(x, p)),
 * 3 rescale (p * x * std(cond) / std(x) + (1 - p) * x); each statistic is over the whole batch tensor.  h_bounds: HOST
 * (3,2) float64 box [lo, hi] per coordinate that clamps every predicted position (the reference's bounds[0]), or NULL.
 * d_pos_uncond_traj (S,N,3) / d_v_uncond_traj (S,N,C) f32 DEVICE receive the raw unconditional predictions, or NULL; the
 * pos_cond / v_cond trajectories of shapemol_traj keep the raw conditional ones, v0_traj the thresholded logits.
 * guide_stren = 0 switches guidance off.  Mesh or point-cloud guidance, when set, take precedence (the reference's elif). */
int shapemol_set_cfg(shapemol_ctx *ctx, double guide_stren, int32_t threshold_type, double p, const double *h_bounds,
                     float *d_pos_uncond_traj, float *d_v_uncond_traj);

/* The same with one strength and one box per GROUP of molecules: group g is molecules [h_mol_off[g], h_mol_off[g + 1]) of the
 * batches to come (HOST offsets, G + 1 of them: start at 0, do not decrease; _sample requires n_mols == h_mol_off[G]).  Per
 * step and group, x = (1 + w_g) * cond - w_g * uncond with h_guide_stren[g] = w_g (HOST, finite), threshold_CFG with the
 * statistic taken over THAT GROUP's elements only -- bit for bit the statistic of a one-group chain of the group's slice,
 * whatever the other groups hold -- and the positions clamped into the group's box: h_bounds is HOST (G,3,2) float64 or NULL,
 * a row that starts with NaN means no clamp for that group.  threshold_type and p are one per chain.  A group with w_g = 0
 * consumes its raw conditional prediction: no threshold, no clamp (the reference's else branch).  At most 256 groups; more are
 * refused, as are offsets or strengths that do not validate (the message names the group).  While a set is installed it takes the
 * place of shapemol_set_cfg's scalars.  n_groups = 0, or every strength 0, removes the set: the chains are unguided.  The
 * strengths, boxes and group boundaries live in device memory: a captured step depends on (n_atoms, n_mols, threshold_type, p,
 * n_groups) only.  shapemol_debug_read "cfg_group_stat" gives the statistics of the last step of the last chain that ran with a set, (G,2) f32:
 * positions | logits (also after the set has been removed). */
int shapemol_set_cfg_groups(shapemol_ctx *ctx, int32_t n_groups, const int64_t *h_mol_off, const double *h_guide_stren,
                            int32_t threshold_type, double p, const double *h_bounds, float *d_pos_uncond_traj,
                            float *d_v_uncond_traj);

/* Input validation happens on the device (no host synchronisation in _score/_sample): an unsorted or
 * out-of-range d_batch, an atom type outside [0, num_classes) or a time step outside [0, num_timesteps)
 * sets a sticky flag (the offending index is clamped, so nothing is read or written out of bounds).
 * shapemol_status synchronises the device and returns non-zero (message in shapemol_last_error) if the
 * last _score/_sample on this context saw such an input, an activation beyond the fp16 range of the two-piece f16 node
 * kernels (option node_f16), a timed-out grid barrier (vn_fuse = 1) or too few within-atoms for mesh guidance;
 * flags_out (may be NULL) receives the eight raw flags {barrier, batch, atom type, time step, fp16 range, span, mesh, 0}.
 * The reference raises from the corresponding torch indexing ops (models/molopt_score_model.py:292-301). */
int shapemol_status(shapemol_ctx *ctx, int32_t *flags_out);
/* The same, synchronising only `stream` (the one the last _score/_sample of this context was enqueued on) instead of the whole
 * device: chains of other contexts running beside it are not waited for. */
int shapemol_status_stream(shapemol_ctx *ctx, int32_t *flags_out, void *stream);

/* Evaluation-mode batch-norm (the module after .eval(): scripts/train_diffusion.py:172-173 puts it there for validate(),
 * models/shape_vn_layers.py:50-61 then normalises the vector norms with BatchNorm1d's running statistics instead of the
 * batch's).  h_mean, h_var: HOST [num_layers][n_heads] float32, the buffers
 * refine_net.base_block.{l}.h2x_layers.0.shape_linear.batchnorm.bn.running_{mean,var}; count = num_layers * n_heads.
 * Takes effect with shapemol_set_option(ctx, "bn_eval", 1); training mode (the default, and what sampling uses: the
 * reference never leaves it while sampling) keeps using the statistics of the batch.  The running statistics
 * are read, never updated (no training step on this path). */
int shapemol_set_bn_running(shapemol_ctx *ctx, const float *h_mean, const float *h_var, int64_t count);

/* argmax_c( logits[n,c] - log(-log(u[n,c] + 1e-30) + 1e-30) ); d_u NULL -> device Philox(seed). */
int shapemol_log_sample_categorical(shapemol_ctx *ctx, const float *d_logits, const float *d_u,
                                    int64_t n_rows, int32_t n_classes, uint64_t seed,
                                    int64_t *out_index, void *stream);

/* ---- frozen shape encoder ------------------------------------------------------------
 * VN_DGCNN_Encoder.forward (models/shape_pointcloud_modelAE.py:207-255) with get_graph_feature_cross / dense knn
 * (models/shape_vn_layers.py:257-292): point clouds (B,N,3) -> shape latents (B,latent_dim,3), the `shape_emb` the
 * diffusion model is conditioned on (utils/shape.py:240-283).  Batch-norm runs on batch statistics, as the reference's
 * auto-encoder does (it is never put in eval mode).  hidden_dim 128, num_k 20 (the shipped checkpoint's config).
 * weights (HOST, float32, shapemol_se_weight_count of them): conv_pos {map_to_feat (C,2), bn weight (C), bn bias (C),
 * map_to_dir (C,2)}; per block {map_to_feat (C,2C), bn weight, bn bias, map_to_dir (C,2C)}; conv_c {map_to_feat
 * (latent,L*C), bn weight (latent), bn bias (latent), map_to_dir (L*C)}. */
typedef struct shapemol_se_ctx shapemol_se_ctx;
size_t shapemol_se_weight_count(int32_t hidden_dim, int32_t latent_dim, int32_t layer_num);
int shapemol_se_create(int32_t hidden_dim, int32_t latent_dim, int32_t layer_num, int32_t num_k, const float *weights,
                       size_t n_weights, int device, shapemol_se_ctx **out);
void shapemol_se_destroy(shapemol_se_ctx *ctx);
/* d_points (B,N,3) f32 DEVICE; d_out (B,latent_dim,3) f32 DEVICE.  1 <= B <= 65535, B*N <= 2^24, and N a multiple of 16 in
 * [32, shapemol_se_max_points(ctx)]: the kNN needs N >= num_k = 20, and keeps the 16 x N distances of a row block in LDS, so the
 * largest N is the device's dynamic LDS per workgroup / 64 bytes, read from the device at creation (2560 where a workgroup can have
 * 160 KiB).  Anything else is refused with a message before any allocation or launch. */
int shapemol_se_encode(shapemol_se_ctx *ctx, const float *d_points, int64_t n_shapes, int64_t n_points, float *d_out, void *stream);
int64_t shapemol_se_max_points(const shapemol_se_ctx *ctx);
/* Diagnostics (tests only).  _debug_read copies one workspace buffer of the last _encode to HOST memory after a device synchronise;
 * n_bytes must be the buffer's exact size for the last encode's P = B*N points:
 *   SHAPEMOL_SE_IDX (P,20) i32 neighbours inside the shape, SHAPEMOL_SE_H0 (P,C,3) f32 conv_pos output, SHAPEMOL_SE_HCAT (P,L,C,3) f32
 *   the blocks' outputs, SHAPEMOL_SE_Y (P,4C,3) f32 the per-point products [Yf1|Yf2|Yd1|Yd2], SHAPEMOL_SE_XX (P) f32 squared feature norms,
 *   SHAPEMOL_SE_PD (P,latent_dim+1,3) f32 conv_c products and the shared direction.
 * idx, y and xx are overwritten by each block: _debug_stop_after(ctx, l) makes the following encodes return after block l (0: after
 * conv_pos, so idx is conv_pos's; l: blocks 0..l-1 have run, idx / xx / y are those of block l-1 and hcat holds slices 0..l-1),
 * without touching d_out; -1 restores the full encode. */
enum { SHAPEMOL_SE_IDX = 0, SHAPEMOL_SE_H0 = 1, SHAPEMOL_SE_HCAT = 2, SHAPEMOL_SE_Y = 3, SHAPEMOL_SE_XX = 4, SHAPEMOL_SE_PD = 5 };
int shapemol_se_debug_stop_after(shapemol_se_ctx *ctx, int32_t n_blocks);
int shapemol_se_debug_read(shapemol_se_ctx *ctx, int32_t what, void *h_dst, size_t n_bytes);
/* Training the encoder: every parameter's gradient; none to the points, none through the neighbour lists.
 * Deterministic: no floating-point atomics, the latent and every gradient are bit-identical from run to run.
 * _load_weights repacks the context's weights from d_weights (DEVICE, the flat vector in the order of _create's `weights`) with a
 * kernel on `stream`: after an optimiser step no host packing and no new context.
 * _train_forward is _encode with batch statistics summed in a fixed order, and leaves what the backward needs in CALLER-OWNED
 * device buffers (a later forward on the context cannot touch them), L = layer_num, P = B*N:
 *   d_idx (L+1,P,20) i32 the neighbour lists of conv_pos and of every block; d_h0 (P,C,3); d_hcat (P,L,C,3); d_pd (P,latent+1,3);
 *   d_stats (L+2,2,256) f64: per stage (conv_pos, the blocks, conv_c) the batch mean and the biased batch variance per channel.
 * _train_backward takes them back with the latent's gradient d_grad_out (B,latent,3) -- or, for a staged check, d_grad_hcat (P,L,C,3),
 * the gradient at conv_c's input, with conv_c skipped and its gradients zero; exactly one of the two is non-NULL -- and writes
 * d_grad_w, shapemol_se_weight_count floats in the weights' order.  Y = W' h is recomputed per block, not saved.
 * d_masks (diagnostic, may be NULL): (L+2,P,256) i32, per stage the leaky-ReLU branches the backward took: for conv_pos and the blocks
 * bit kk of [i][c] is set where edge (i, kk) of channel c had dot < 0, for conv_c [p][m] is 1 where row m had; written only by
 * the stages that run.  The training calls do not feed _debug_read, which keeps referring to the last _encode, and
 * _debug_stop_after does not shorten them.
 * Both calls work in d_ws, a caller-owned device buffer of at least _train_workspace(ctx, B, N) bytes aligned to 256 bytes, whose
 * contents mean nothing between calls.  Shapes as _encode; refusals come with a message before any launch. */
int shapemol_se_load_weights(shapemol_se_ctx *ctx, const float *d_weights, size_t n_weights, void *stream);
size_t shapemol_se_train_workspace(const shapemol_se_ctx *ctx, int64_t n_shapes, int64_t n_points);
int shapemol_se_train_forward(shapemol_se_ctx *ctx, const float *d_points, int64_t n_shapes, int64_t n_points, int32_t *d_idx, float *d_h0,
                              float *d_hcat, double *d_stats, float *d_pd, float *d_out, void *d_ws, size_t ws_bytes, void *stream);
int shapemol_se_train_backward(shapemol_se_ctx *ctx, const float *d_points, int64_t n_shapes, int64_t n_points, const int32_t *d_idx,
                               const float *d_h0, const float *d_hcat, const double *d_stats, const float *d_pd, const float *d_grad_out,
                               const float *d_grad_hcat, float *d_grad_w, int32_t *d_masks, void *d_ws, size_t ws_bytes,
                               void *stream);

/* ---- shape decoder: the auto-encoder's implicit field --------------------------------------------------------------
 * DecoderInner.forward (models/shape_pointcloud_modelAE.py:21-103, blocks: ResnetBlockFC, models/shape_vn_layers.py:210-252):
 * the signed distance (SHAPEMOL_SD_SIGNEDDIST, no output activation) or occupancy (SHAPEMOL_SD_OCCUPANCY, sigmoid) that a
 * shape latent z (latent,3) encodes, at query points.  ReLU activations (PointCloud_AE never sets `leaky`).  hidden 128,
 * latent 1..256, layer_num 1..8; anything else, or a wrong weight count, is refused with a message that names the limit.
 * weights (HOST, float32, shapemol_sd_weight_count of them): z_in.map_to_feat (latent,latent); fc_in weight (H,2*latent+1),
 * bias (H); per block {fc_0 weight (H,H), bias (H), fc_1 weight (H,H), bias (H)}; fc_out weight (H), bias (1). */
typedef struct shapemol_sd_ctx shapemol_sd_ctx;
enum { SHAPEMOL_SD_SIGNEDDIST = 0, SHAPEMOL_SD_OCCUPANCY = 1 };
size_t shapemol_sd_weight_count(int32_t hidden, int32_t latent, int32_t layer_num);
int shapemol_sd_create(int32_t hidden, int32_t latent, int32_t layer_num, int32_t loss_type, const float *weights,
                       size_t n_weights, int device, shapemol_sd_ctx **out);
void shapemol_sd_destroy(shapemol_sd_ctx *ctx);
/* d_p (n_points,3) f32, d_z (n_shapes,latent,3) f32, d_out (n_points) f32, all DEVICE.  The shape of point i is
 * d_shape_of[i] (int32 DEVICE, any order; clamped into [0, n_shapes) by the kernel -- validate it before the call), or,
 * with d_shape_of null, i / points_per_shape (then n_points must be n_shapes * points_per_shape).  A point's result does
 * not depend on the other points of the call.  n_shapes in 1..65535 and n_points < 2^31, else refused with a message
 * before any allocation or launch; n_points == 0 returns 0 without a launch.
 * A context holds the per-shape workspace (z_inv, G, c) that every decode rewrites: use it from one stream at a time (order
 * decodes on different streams with events), or create one context per stream.  The first decode with more shapes than any
 * before it grows that workspace, which synchronises the device once. */
int shapemol_sd_decode(shapemol_sd_ctx *ctx, const float *d_p, const int32_t *d_shape_of, int64_t n_points,
                       int64_t points_per_shape, const float *d_z, int64_t n_shapes, float *d_out, void *stream);
/* The entry points of the decoder's gradient are named shapemol_field_*, not shapemol_sd_*: the set of shapemol_sd_* functions
 * is a fixed list that tests/test_shape_decoder_cpu.py compares this header against, and these came later.  They take the same
 * shapemol_sd_ctx.
 * The field's value and its gradient with respect to the query point in one pass: d_grad (n_points,3) f32 DEVICE =
 * d out / d p, by reverse mode through the kept ReLU masks (mask = input > 0, torch's convention at 0); d_out as
 * shapemol_sd_decode writes it, bit for bit, or NULL.  Contract, limits and refusals: those of shapemol_sd_decode. */
int shapemol_field_decode_grad(shapemol_sd_ctx *ctx, const float *d_p, const int32_t *d_shape_of, int64_t n_points,
                            int64_t points_per_shape, const float *d_z, int64_t n_shapes, float *d_out, float *d_grad,
                            void *stream);
/* One always-applied pass of the reference's gradient shape guidance (models/molopt_score_model.py:592-615), in place on
 * d_pos (n_atoms,3) f32 DEVICE: with d the field of shape d_batch[i] at atom i and T the atom count of its molecule,
 *     p <- p - grad_lr * (min(d, 0.5) - 0.5) * (1[d < 0.5] / T) * grad_p d
 * (atoms with d >= 0.5 stay).  d_batch (n_atoms) int64 DEVICE, SORTED, values in [0, n_shapes) (clamped by the kernel --
 * validate before the call).  n_shapes in 1..65535, n_atoms <= 2^27, grad_lr finite, else refused.  Uses the context's
 * workspace like a decode. */
int shapemol_field_guide(shapemol_sd_ctx *ctx, float *d_pos, const int64_t *d_batch, int64_t n_atoms, const float *d_z,
                      int64_t n_shapes, double grad_lr, void *stream);
/* Gradient shape guidance inside the chains of a sampling context: the following shapemol_sample calls apply the pass above
 * to the predicted x0 of every step with t > grad_step, each molecule against the field of ITS OWN row of the chain's
 * d_shape (so the decoder's latent must equal the model's shape_dim).  The per-shape prologue runs once per chain; the
 * guidance launch is part of the captured step.  Precedence follows the reference's if / elif: a mesh, then a point cloud,
 * then this, then classifier-free guidance.  An installed decoder takes its branch even when grad_step >= num_timesteps - 1
 * lets no step be guided: the chain is then the unguided one, and classifier-free guidance is not reached either, as behind the
 * reference's `elif`.  sd = NULL removes it.  Refused with a message: a decoder on another device,
 * latent != shape_dim, a grad_lr that is not finite.
 * The decoder context is BORROWED: it must outlive every chain of `ctx` that was enqueued while it was installed, and it
 * serves one stream at a time -- a decode, decode_grad or guide on it while such a chain is in flight must be ordered behind
 * the chain by the caller. */
int shapemol_set_field_guidance(shapemol_ctx *ctx, shapemol_sd_ctx *sd, double grad_lr, int32_t grad_step);
/* Points a workgroup of the decode kernel takes per iteration (tests derive their edge shapes from it), and of the kernel
 * behind _decode_grad / _guide (a divisor of the former). */
int64_t shapemol_sd_tile(const shapemol_sd_ctx *ctx);
int64_t shapemol_field_grad_tile(const shapemol_sd_ctx *ctx);
/* Training the decoder.  One call is the forward and the whole backward of a loss whose gradient with respect to the field is
 * d_upstream: dense form only (shape b owns points b * points_per_shape .. (b + 1) * points_per_shape - 1 of d_p).
 *   d_upstream (B T) f32 DEVICE  dLoss / d out (for occupancy the kernel multiplies by s (1 - s) itself)
 *   d_out      (B T) f32 DEVICE or NULL: the value, bit for bit shapemol_sd_decode's
 *   d_grad_p   (B T,3) or NULL, d_grad_z (B,latent,3), d_grad_weights (shapemol_sd_weight_count floats, in the order of the
 *              weights of shapemol_sd_create): every element is written
 * Deterministic: no atomics, every sum over points and shapes in a fixed order; two calls on the same inputs give the same bits.
 * The points are taken in chunks of chunk_points (a multiple of shapemol_field_train_tile; 0 = one tile per compute unit); the
 * workspace is sized by the chunk, not by B T, and like the per-shape workspace it grows behind a device synchronise and
 * serves one stream at a time.  Refused: what shapemol_sd_decode refuses, a NULL upstream, a chunk that is no multiple of the
 * tile. */
int shapemol_field_train(shapemol_sd_ctx *ctx, const float *d_p, int64_t n_shapes, int64_t points_per_shape, const float *d_z,
                         const float *d_upstream, float *d_out, float *d_grad_p, float *d_grad_z, float *d_grad_weights,
                         int64_t chunk_points, void *stream);
/* New weights for an existing context from DEVICE memory: d_weights holds shapemol_sd_weight_count floats in the order of
 * shapemol_sd_create.  One kernel on `stream` rewrites the forward and transposed images, the biases, w_0 and w_out; nothing
 * touches the host or synchronises.  The context's identity advances, so a chain step captured with the old field
 * (shapemol_set_field_guidance) is captured again.  One stream at a time, as every use of the context. */
int shapemol_field_load_weights(shapemol_sd_ctx *ctx, const float *d_weights, size_t n_weights, void *stream);
int64_t shapemol_field_train_tile(const shapemol_sd_ctx *ctx);
/* Diagnostics (tests only): the per-shape prologue of the last _decode, copied to HOST memory after a device synchronise;
 * n_bytes must be the exact size for its B = n_shapes: SHAPEMOL_SD_ZINV (B,latent) f32 z_inv = sum_xyz z * z_in(z),
 * SHAPEMOL_SD_G (B,H,3) f32 G = W_z z and SHAPEMOL_SD_C (B,H) f32 c = W_inv z_inv + bias of the factored fc_in
 * fc_in(feature) = w_0 |p|^2 + G p + c. */
enum { SHAPEMOL_SD_ZINV = 0, SHAPEMOL_SD_G = 1, SHAPEMOL_SD_C = 2 };
int shapemol_sd_debug_read(shapemol_sd_ctx *ctx, int32_t what, void *h_dst, size_t n_bytes);

/* ---- training building blocks (the operators of a layer, forward and backward) ---------------
 * The MLP block of models/common.py:47-67 -- y = W2 relu(LayerNorm(W1 x + b1)) + b2, eps 1e-5, affine LayerNorm -- forward
 * with the quantities its backward needs, and the backward: what torch.autograd does for the 58 MLPs of one score
 * evaluation when scripts/train_diffusion.py:135-147 calls loss.backward().  fp32 arithmetic (fp32 MFMA products), device
 * pointers, row-major: x (rows,k_in), w1 (hidden,k_in), b1/gamma/beta (hidden), w2 (n_out,hidden), b2 (n_out), y (rows,n_out).
 * _forward also writes xhat (rows,hidden) = the normalised pre-activation, rstd (rows) and act (rows,hidden) = the ReLU output
 * (xhat and rstd must be kept for _backward; act may be kept and handed back, or dropped: _backward recomputes it from xhat when
 * d_act is NULL).
 * _backward: dy (rows,n_out) -> dx (rows,k_in; may be NULL), dw1, db1, dgamma, dbeta, dw2, db2 (OVERWRITTEN, not
 * accumulated); d_work: shapemol_mlp_backward_workspace() floats.  Reductions over the rows are deterministic. */
size_t shapemol_mlp_backward_workspace(int64_t rows, int32_t k_in, int32_t hidden, int32_t n_out);
int shapemol_mlp_forward(const float *d_x, int64_t rows, int32_t k_in, int32_t hidden, int32_t n_out, const float *d_w1,
                         const float *d_b1, const float *d_gamma, const float *d_beta, const float *d_w2, const float *d_b2,
                         float *d_y, float *d_xhat, float *d_rstd, float *d_act, void *stream);
int shapemol_mlp_backward(const float *d_x, const float *d_dy, int64_t rows, int32_t k_in, int32_t hidden, int32_t n_out,
                          const float *d_w1, const float *d_gamma, const float *d_beta, const float *d_w2, const float *d_xhat,
                          const float *d_rstd, const float *d_act, float *d_dx, float *d_dw1, float *d_db1, float *d_dgamma, float *d_dbeta,
                          float *d_dw2, float *d_db2, float *d_work, size_t work_floats, void *stream);

/* The same block on edge rows whose input is the reference's concatenation [r_e | h_i | h_j | s_i] for edge e = (centre i = dst[e],
 * neighbour j = src[e]) (models/uni_transformer.py:60-66 / :131-137: hk_func, hv_func, xk_func, xv_func): r (n_edges, k_edge) edge
 * features, h (n_nodes, k_node) atom features, s (n_nodes, k_shape) per-atom shape embedding (k_shape may be 0, d_s NULL),
 * W1 (hidden, k_edge + 2 k_node + k_shape) with the reference's column order.  The concatenated rows are never formed: the
 * first Linear is evaluated as an edge term plus per-atom terms (pd, ps: (n_nodes, hidden) scratch), and the backward sums over
 * each atom's edges before its per-atom products.  Edges must be grouped by centre atom (ptr_dst: n_nodes + 1 CSR offsets);
 * perm_src / ptr_src list the edges grouped by neighbour atom (perm_src[t] = edge index).  Outputs and workspace as in
 * shapemol_mlp_*; dW1 is written whole, dr / dh / ds are the gradients of r / h / s. */
size_t shapemol_edge_mlp_backward_workspace(int64_t n_edges, int64_t n_nodes, int32_t k_edge, int32_t k_node, int32_t k_shape, int32_t hidden, int32_t n_out);
int shapemol_edge_mlp_forward(const float *d_r, const float *d_h, const float *d_s, const int64_t *d_dst, const int64_t *d_src, int64_t n_edges,
                              int64_t n_nodes, int32_t k_edge, int32_t k_node, int32_t k_shape, int32_t hidden, int32_t n_out, const float *d_w1,
                              const float *d_b1, const float *d_gamma, const float *d_beta, const float *d_w2, const float *d_b2, float *d_y,
                              float *d_xhat, float *d_rstd, float *d_act, float *d_pd, float *d_ps, void *stream);
int shapemol_edge_mlp_backward(const float *d_r, const float *d_h, const float *d_s, const int64_t *d_ptr_dst, const int64_t *d_perm_src,
                               const int64_t *d_ptr_src, const float *d_dy, int64_t n_edges, int64_t n_nodes, int32_t k_edge, int32_t k_node,
                               int32_t k_shape, int32_t hidden, int32_t n_out, const float *d_w1, const float *d_gamma, const float *d_beta,
                               const float *d_w2, const float *d_xhat, const float *d_rstd, const float *d_act, float *d_dr, float *d_dh, float *d_ds, float *d_dw1,
                               float *d_db1, float *d_dgamma, float *d_dbeta, float *d_dw2, float *d_db2, float *d_work, size_t work_floats, void *stream);

/* The coordinate update's vector-neuron block on the training path: VNLinearLeakyReLU with VNBatchNorm
 * (models/shape_vn_layers.py:41-61, 95-110) applied to [x_n | o3_n | shape_mol(n)] and averaged over the output channels
 * (models/uni_transformer.py:157-160).  x (n_atoms, 3), o3 (n_atoms, rows_o, 3), shape (n_molecules, rows_s, 3), batch (n_atoms)
 * molecule index of every atom, wf / wd (channels, 1 + rows_o + rows_s), out (n_atoms, 3).  training != 0: batch statistics
 * (running estimates, when given, updated with momentum 0.1 as nn.BatchNorm1d does); 0: the running estimates.  pf, dir
 * (n_atoms, channels, 3) and stats (2, channels) are kept for the backward; nrm (n_atoms, channels) is scratch.  _backward: dx,
 * do3, dwf, dwd (channels, 1 + rows_o + rows_s each), dbn_w, dbn_b from gout (n_atoms, 3); no gradient for shape (it comes
 * from the frozen encoder). */
size_t shapemol_vn_backward_workspace(int64_t n_atoms, int32_t rows_o, int32_t rows_s, int32_t channels);
int shapemol_vn_forward(const float *d_x, const float *d_o3, const float *d_shape, const int64_t *d_batch, int64_t n_atoms, int32_t rows_o,
                        int32_t rows_s, int32_t channels, const float *d_wf, const float *d_wd, const float *d_bn_w, const float *d_bn_b,
                        float *d_run_mean, float *d_run_var, int32_t training, float *d_out, float *d_pf, float *d_dir, float *d_stats,
                        float *d_nrm, void *stream);
int shapemol_vn_backward(const float *d_x, const float *d_o3, const float *d_shape, const int64_t *d_batch, int64_t n_atoms, int32_t rows_o,
                         int32_t rows_s, int32_t channels, const float *d_wf, const float *d_wd, const float *d_bn_w, const float *d_bn_b,
                         const float *d_pf, const float *d_dir, const float *d_stats, int32_t training, const float *d_gout, float *d_dx,
                         float *d_do3, float *d_dwf, float *d_dwd, float *d_dbn_w, float *d_dbn_b, float *d_work, size_t work_floats, void *stream);

/* The attention of one layer on the training path (models/uni_transformer.py:71-81 / :141-151): for every centre atom i, whose
 * incoming edges are e in [ptr[i], ptr[i+1]) (edges grouped by centre), and head h: logits <q_i[h], k_e[h]> / sqrt(dh), softmax
 * over the atom's edges, out_i[h][:] = sum_e alpha_e vals_e[h][:].  q (n_atoms, heads*dh), k (n_edges, heads*dh), vals
 * (n_edges, heads, width) with width = dh (x2h) or 3 (h2x: value times relative position); dh, width <= 8.  _backward writes
 * dq, dk, dvals (every edge belongs to exactly one atom: no accumulation, deterministic). */
int shapemol_seg_attention_forward(const float *d_q, const float *d_k, const float *d_vals, const int64_t *d_ptr, int64_t n_atoms,
                                   int32_t heads, int32_t dh, int32_t width, float *d_out, void *stream);
int shapemol_seg_attention_backward(const float *d_q, const float *d_k, const float *d_vals, const int64_t *d_ptr, const float *d_dout,
                                    int64_t n_atoms, int32_t heads, int32_t dh, int32_t width, float *d_dq, float *d_dk, float *d_dvals,
                                    void *stream);

/* ---- diagnostics (used by the parity tests and the bench; not needed by a caller) ---- */
/* (options marked "_sample only" do not affect _score)
 * options: "first_step" (the following _sample calls resume a chain at reverse step v, i.e. at t = T-1-v, from the
 *                        state given as d_init_pos / d_init_v; noise and trajectory rows stay indexed from 0; default 0.
 *                        Used by the windowed full-length parity test; the reference always starts at T-1),
 *          "stop_layer" (run only the first v layers of the next _score; -1 = all),
 *          "edge_bf16"  (3 = fused key/value edge kernel on two-piece f16 operands, both MLP images resident;
 *                        2 = streaming kernels on exactly split bf16 operands (three pieces = the 24 bits of fp32, six products):
 *                            weights stationary in the registers of consumer waves, producer waves stream edge tiles through
 *                            LDS (sm_edge_stream.h; k <= 16) -- the reference-precision path;
 *                        1 = fused phase kernel on exactly split bf16 operands (weight swap between the phases; k <= 16),
 *                        0 = fp32-MFMA edge kernels),
 *          "node_f16"   (1 = node kernels (prologue, chain, per-node products) on two-piece f16 operands [default]: the
 *                        residual stream then passes through fp16 pieces, |x| >= 6e4 raises a status flag;
 *                        0 = the same kernels on exactly split bf16 operands, six products per term),
 *          "feat_f16"   (1 = "f16 features": every matrix product of the f16 kernels on the leading f16 piece of both operands
 *                        only -- one product per term instead of three, 11 significand bits in the operands; accumulation,
 *                        LayerNorm, softmax, coordinates, batch statistics stay fp32.  A reduced-precision throughput mode
 *                        (forward error ~1e-3), outside the parity gates; 0 = two-piece operands [default]),
 *          "lin_bf16", "chain_bf16" (1 = node kernels on the matrix cores with split operands [default],
 *                        0 = fp32-MFMA node kernels),
 *          "edge_tiles" (f16 edge kernels when the waves have several jobs (batches beyond ~6k atoms, k > 16): 1 = one looping
 *                        launch, eight waves per workgroup over consecutive jobs with the next job's rows prefetched,
 *                        0 = sliced launches of the one-job kernel, -1 = automatic (= 1) [default]; k > 16 runs every atom
 *                        as two 16-slot tiles merged by an online-softmax combine kernel in either form),
 *          "max_mol_atoms" (_sample only: largest molecule, in atoms, of the batches of the following chains; 0 = unknown [default].  With it
 *                        the coordinate update of every layer but the last runs in the prologue of the next layer's x2h
 *                        kernel (each workgroup recomputes the coordinates of the molecules its atoms belong to) instead
 *                        of as a launch of its own; a value smaller than the truth raises a status flag.  Does not touch the
 *                        captured graph unless it changes that decision),
 *          "vn_fold"    (1 = fold as above when max_mol_atoms allows [default], 0 = always launch vn_apply),
 *          "vn_fuse"    (2 = VN-linear + batch-norm statistics in the epilogue of the h2x attention, vn_apply as its
 *                        own launch [default]; 1 = the whole coordinate update behind h2x with an in-kernel grid
 *                        barrier (no faster: measured); 0 = separate vn_stats / vn_apply launches),
 *          "bn_eval"    (1 = evaluation-mode batch-norm: the running statistics of shapemol_set_bn_running; 0 = the
 *                        statistics of the batch [default, and what the reference's sampling runs with]),
 *          "x2h_chain"  (1 = x2h attention and node stage of a layer in one launch when every wave has one job in a
 *                        single launch (up to ~6k atoms) [default], 0 = separate launches),
 *          "graph_fuse" (1 = kNN graph + edge weights in one launch when max_mol_atoms is known and <= 128 [default]),
 *          "ddpm_fold"  (_sample only: 1 = the last layer's coordinate update inside the posterior-step kernel when the
 *                        fold above applies and no guidance is set [default]),
 *          "prologue_tab" (1 = the node prologue of an evaluation (h0, layer-0 queries, layer-0 per-node products) is a gather from
 *                        tables over every (timestep, atom type) pair, built once per context and node precision mode by the
 *                        per-atom prologue kernel [default]; 0 = that per-atom kernel at every evaluation.  Same results to the
 *                        bit; tuning / A/B),
 *          "edge_waves" (waves per workgroup of the edge kernels, 1..12; 0 = automatic: ceil(jobs / CUs) [default]; a
 *                        value other than 0 also selects the separate launches),
 *          "lin_waves"  (1..16 waves per workgroup of node_linear_kernel, tuning),
 *          "x2h_out_fuse" (exact streaming mode with the two-level node form, k <= 16: 1 = h' = h + MLP_out([att | h]) in the tail of the
 *          x2h kernel instead of a node_out6_kernel launch while a workgroup owns at most 96 atoms [default], 2 = whatever it owns,
 *          0 = node_out6_kernel; same bits), "stream_chunk" (tiles per workgroup of the streaming edge kernels, 0 = automatic
 *          [default]; for tests),
 *          "node_levels" (exact-mode node kernels: 1 = the node stage of a layer by dependency level -- node_out6_kernel (h' only),
 *                        then node_after6_kernel (follow-up MLPs and per-node products of h' side by side in one grid) [default];
 *                        0 = node_chain6_kernel + node_linear6_kernel.  Same results to the bit; tuning / A/B),
 *          "after_order" (node_after6_kernel's grid: 0 = follow-up jobs first, 1 = interleaved with the linear jobs in
 *                        proportion, 2 = linear jobs first [default]; tuning, same results),
 *          "after_waves" (1..16 waves of node_after6_kernel's linear jobs [default 16]; the workgroup has max(H / 16,
 *                        after_waves) waves, and up to 8 let two workgroups share a CU; tuning, same results),
 *          "after_lin_wgs" (workgroups aimed at for node_after6_kernel's linear jobs, 0 = automatic [default]; tuning, same results),
 *          "stream_whole_rounds" (streaming edge kernels, k <= 16: 1 = tiles per workgroup rounded up to whole rounds of two; 0 =
 *                        ceil(tiles / CUs), the last round of an odd count has one tile [default]; tuning, same results),
 *          "stamps", "kstamp_sel" (clock-stamp diagnostics; only meaningful in the --stamps build).
 * Changing an option invalidates a captured graph (the next _sample re-captures). */
int shapemol_set_option(shapemol_ctx *ctx, const char *name, int64_t value);
/* Diagnostic of the parity tests: pin the kNN graph of the following _sample calls at given (reverse step, atom) pairs to given
 * neighbour lists (the reference's own, recorded where its k-th / (k+1)-th choice is closer than a float32 implementation can
 * reproduce: models/uni_transformer.py:446-473 builds one graph per score evaluation, and a flipped neighbour sends the molecule
 * down another trajectory for good).  h_off: HOST [n_steps + 1] CSR offsets of the pins of reverse step s = 0 .. n_steps - 1
 * (s = num_timesteps - 1 - t); h_atom [n_pins] atom index; h_nbr [n_pins][k] neighbour indices (global atom indices, the
 * reference's order).  n_pins = 0 removes the pins.  While pins are set the graph is built by the separate kNN / edge-weight
 * launches (the pinned rows are overwritten between them). */
int shapemol_set_knn_pins(shapemol_ctx *ctx, const int32_t *h_off, int32_t n_steps, const int32_t *h_atom, const int32_t *h_nbr,
                          int64_t n_pins, int32_t k);
/* Diagnostic (host only, no device needed): the exact three-way bf16 split of the default precision mode -- every matrix operand x is
 * carried as hi + mid + lo with hi = x truncated to bf16, mid = (x - hi) truncated, lo = x - hi - mid (8 + 8 + 8 significand bits,
 * fp32 exponent range), so that x == hi + mid + lo EXACTLY for every fp32 value of magnitude 2^-110 (7.7e-34) and above (below that the
 * third piece falls under bf16's smallest subnormal and the error is bounded by 2^-133) (fp32 nn.Linear operands of the reference:
 * models/common.py:47-67).  pieces: three bf16 bit patterns.  tests/test_host.py checks the identity over random and edge values. */
void shapemol_debug_split_exact(float x, uint16_t *pieces);
/* Diagnostic: the statistic stage of ONE classifier-free guidance step on caller-supplied predictions, under the setting that
 * shapemol_set_cfg or shapemol_set_cfg_groups installed -- exactly what a chain launches for it: the histograms cleared, with
 * groups their table from d_batch (n_atoms,) i64 DEVICE, then the partial-sum or the three radix-select launches and the
 * finalize launch over d_pos_cond / d_pos_uncond (n_atoms,3) and d_v_cond / d_v_uncond (n_atoms,num_classes) f32 DEVICE.  The
 * result stays where a chain leaves it: shapemol_debug_read "cfg_stat" (2,) f32, with groups "cfg_group_stat" (G,2) f32
 * (threshold_type 0 has no statistic: nothing is launched).  Enqueued on `stream`, no synchronisation.  Refused before any
 * launch: a null pointer, n_atoms < 1, n_mols < 1 or > n_atoms, n_atoms * num_classes >= 2^31, no classifier-free setting
 * installed (or a mesh, a cloud or a field installed, which take precedence), a group set that does not cover n_mols.  The
 * workspace grows as for _sample (a growth drops the captured steps; the next chain captures again); chains before and after
 * are otherwise untouched.  tests/test_gpu_cfg_stats.py gates the statistic kernels through it on crafted tensors. */
int shapemol_debug_cfg_stats(shapemol_ctx *ctx, const float *d_pos_cond, const float *d_pos_uncond, const float *d_v_cond,
                             const float *d_v_uncond, const int64_t *d_batch, int64_t n_atoms, int64_t n_mols, void *stream);
/* Copy an internal device buffer of the last _score to HOST memory (synchronises the device).
 * names: "nbr" (N,KP) i32, "ew" (N,KP) f32, "h" (N,H), "x" (N,3), "pre" (N,4H), "q" (N,H),
 *        "h0" (N,H), "q_x" (N,H), "pre0" (N,4H), "add0" (B,4H): the node prologue's outputs and the per-molecule term it adds
 *        (intact after an evaluation with stop_layer = 1),
 *        "att" (N,H), "o3" (N,48), "bnstat" (L,16,2,heads) f64, "dims" (8,) i64,
 *        "captures" (1,) i64 hipGraph captures of this context so far,
 *        "launch" (8,) i64 the launch forms the most recent score evaluation chose (host memory, no synchronise): {chain step?,
 *        fused kNN graph + edge-weight kernel, a coordinate update folded into an x2h kernel, the last one folded into the
 *        posterior kernel, x2h attention + node stage in one launch, streaming edge kernels' tiles per workgroup, their grid
 *        (0, 0 on the other edge kernels), CUs}; after a graph replay: the decisions taken when that step was captured,
 *        "launch_edge" (4,) i64 the edge tiles of that evaluation (host memory): {half-atom tiles used (k > 16), tiles per
 *        attention, combine32_kernel launches issued, floats of a row of the half-tile buffer},
 *        "mesh_group_flags" (G,) i32: per group of the last chain / pass with mesh groups, the steps in which the group was
 *        left unguided for want of within-atoms (status flag 6 says that some group was, this says which and how often).
 * Returns the number of bytes written, or -1. */
int64_t shapemol_debug_read(shapemol_ctx *ctx, const char *name, void *host_dst, size_t max_bytes);
/* ---- shape auto-encoder batches from triangle meshes ---------------------------------------------------------------
 * The reference's ShapeData / collate_fn (datasets/shape_data.py:106-187) and the mesh half of get_pointAE_shape_emb
 * (utils/shape.py:240-284) on the device.  A batch is n_shapes meshes back to back: HOST h_vert_off / h_face_off (n_shapes + 1,
 * starting at 0), h_verts (sum V, 3) float64, h_faces (sum F, 3) int32 with indices relative to the mesh's own vertices.  Per
 * mesh: n_cloud surface points, area-weighted (pytorch3d's rule), rounded to float32; 3 * n_samples uniform candidates in the
 * bounding box grown by 1 on every side; containment by this library's ray parity (the rule of mesh guidance, not trimesh's;
 * meshes are not checked for closedness) and the float64 distance to the nearest cloud point; the FIRST min(n_samples / 2,
 * #inside) inside candidates followed by the first outside ones up to n_samples rows; everything centred on the float32 mean of
 * the cloud.  Limits, refused with a message: n_shapes 1..65535, every mesh >= 1 face, face indices inside the mesh's
 * vertices, finite vertices, n_cloud 1..2048 (the cloud is staged in LDS), n_samples >= 2 -- or 0: clouds, centres and bounds
 * only, d_points / d_values / h_counts may then be null --, loss_type SHAPEMOL_SD_SIGNEDDIST or SHAPEMOL_SD_OCCUPANCY.
 * The check alone touches no device. */
typedef struct shapemol_sdata_ctx shapemol_sdata_ctx;
int shapemol_sdata_check(int64_t n_shapes, const int64_t *h_vert_off, const double *h_verts, const int64_t *h_face_off,
                         const int32_t *h_faces, int64_t n_cloud, int64_t n_samples, int32_t loss_type);
int shapemol_sdata_create(int device, shapemol_sdata_ctx **out);
void shapemol_sdata_destroy(shapemol_sdata_ctx *ctx);
/* Uniforms: DEVICE float64 tables d_cloud_draws (n_shapes, n_cloud, 3) and d_query_draws (n_shapes, 3 * n_samples, 3), each
 * optional; without a table the kernels draw from Philox keyed by (seed, shape, point).  DEVICE float32 outputs: d_cloud
 * (n_shapes, n_cloud, 3) centred, d_points (n_shapes, n_samples, 3) centred, d_values (n_shapes, n_samples) = +d inside / -d
 * outside (signed distance) or 1 / 0 (occupancy), d_centres (n_shapes, 3), d_bounds (n_shapes, 3, 2) = the vertex bounding
 * box minus the centre.  HOST h_counts (n_shapes, 2) int32 = (inside, outside) candidates of every shape.  Optional DEVICE
 * int32 outputs for tests: d_face_idx (n_shapes, n_cloud) the face of every cloud point, d_flags (n_shapes, 3 * n_samples)
 * the containment of every candidate, d_sel (n_shapes, n_samples) the candidate of every row.
 * The call synchronises the stream.  Returns 0; 1 on an error; 2 when some shape has too few outside candidates to fill
 * its rows (the reference's torch.stack fails there): the message names the shapes, h_counts is valid, the rows of those
 * shapes are incomplete, and the context stays usable.  A context serves one stream at a time. */
int shapemol_sdata_build(shapemol_sdata_ctx *ctx, int64_t n_shapes, const int64_t *h_vert_off, const double *h_verts,
                         const int64_t *h_face_off, const int32_t *h_faces, int64_t n_cloud, int64_t n_samples, int32_t loss_type,
                         const double *d_cloud_draws, const double *d_query_draws, uint64_t seed, float *d_cloud, float *d_points,
                         float *d_values, float *d_centres, float *d_bounds, int32_t *h_counts, int32_t *d_face_idx,
                         int32_t *d_flags, int32_t *d_sel, void *stream);

/* ---- molecular surface meshes from atoms and radii ------------------------------------------------------------------
 * What the reference's get_mesh (utils/shape.py:153-162) asks of oddt, under THIS library's rule (not
 * oddt's marching cubes, which is not available to compare with).  A batch is n_mols molecules back to back: HOST h_atom_off
 * (n_mols + 1, starting at 0), centres (sum N, 3) and radii (sum N) float64.  Centres, radii and the probe radius are
 * multiplied by `scaling`; `spacing` h is the grid spacing in those scaled units.  Per molecule, float64 throughout: a grid
 * that reaches 2h beyond every inflated sphere; fA = min_i(|x - c_i| - (r_i + p)) on its nodes; for p > 0 the eroded field
 * g = p - min(d, p + h), d the distance to the nearest node with fA >= 0, else g = fA; the zero level of g (g >= 0: outside) by
 * marching tetrahedra on the six Kuhn tetrahedra of every cell, vertices at t = g0 / (g0 - g1) in (node, edge class) order,
 * faces in (cell, tetrahedron, triangle) order with normals pointing outwards.  The mesh is closed and the same in every run.
 * Limits, refused with a message before any kernel runs: n_mols 1..65535; 1..1024 atoms per molecule; radii > 0, probe_radius
 * >= 0, spacing > 0, scaling > 0, everything finite; ceil((p + h) / h) <= 16; at most 128^3 grid nodes per molecule (so that
 * int32 holds every vertex and face index) and 2^26 per call.  shapemol_msurf_sizes writes up to n of (nodes per molecule,
 * nodes per call, atoms per molecule, stencil, erosion tile edge, nodes per scan block, molecules per call, scan blocks per pass
 * of the per-molecule scan) and returns 8.
 * The check alone touches no device. */
typedef struct shapemol_msurf_ctx shapemol_msurf_ctx;
int shapemol_msurf_sizes(int64_t *out, int32_t n);
int shapemol_msurf_check(int64_t n_mols, const int64_t *h_atom_off, const double *h_centres, const double *h_radii,
                         double probe_radius, double spacing, double scaling);
int shapemol_msurf_create(int device, shapemol_msurf_ctx **out);
void shapemol_msurf_destroy(shapemol_msurf_ctx *ctx);
/* centres / radii: HOST, or DEVICE with inputs_on_device != 0 (they are fetched: the grids are laid out on the host).  HOST
 * outputs: h_counts (n_mols, 2) int32 = (vertices, faces) of every molecule; optional h_lo (n_mols, 3) float64 and h_dims
 * (n_mols, 3) int32 = every grid's corner and node counts; optional h_stage_ms (6) = milliseconds of field, erosion, counting,
 * scan with its host round trip, vertices, faces.  The meshes stay in the context until its next build, back to back in
 * molecule order: float64 vertices (sum V, 3) and int32 faces (sum F, 3) with indices relative to the molecule's own vertices.
 * The call synchronises the stream.  Returns 0, or 1 with a message; a refused batch leaves the context usable. */
int shapemol_msurf_build(shapemol_msurf_ctx *ctx, int64_t n_mols, const int64_t *h_atom_off, const double *centres,
                         const double *radii, int32_t inputs_on_device, double probe_radius, double spacing, double scaling,
                         int32_t *h_counts, double *h_lo, int32_t *h_dims, double *h_stage_ms, void *stream);
/* Copy the first n_items scalars of the last build's vertices (which = 0, float64), faces (1, int32) or node field g (2,
 * float64, the grids back to back) to dst, HOST or DEVICE.  Synchronises the stream. */
int shapemol_msurf_copy(shapemol_msurf_ctx *ctx, int32_t which, void *dst, int64_t n_items, void *stream);

/* ---- geometry scores of sampled molecules: stability and pair distances ------------------------------------------------
 * What the reference's evaluation script asks of analyze.check_stability and eval_bond_length.pair_distance_from_pos_v /
 * get_pair_length_profile, for n_frames frames of one packed batch: n_mols molecules back to back,
 * HOST h_off (n_mols + 1, starting at 0, shared by all frames), N = h_off[n_mols] atoms per frame.  The rule is data:
 * h_thresholds (3, E, E) float64 = bondsK + marginK in pm, formed by the caller in float64; h_allowed (E) the valences;
 * h_class_slot (n_classes) int32 the row of the rule (0 .. E - 1) of every atom class; carbon_slot the row of atomic number 6
 * (-1: the rule has none, no C-C pair); the two histograms' ascending bin edges and cut-offs.  All arithmetic is float64 in
 * the reference's order, d = sqrt((dx*dx + dy*dy) + dz*dz) without FMA contraction; a pair's bond order is 3, 2, 1 or 0 by the
 * nested strict tests 100 * d < threshold1, < threshold2, < threshold3; a pair i < j with d < cut-off adds 1 to the bin
 * np.searchsorted(edges, d, side='left') (C-C: both atoms of the carbon slot).  NaN distances give order 0 and no entry.
 * Molecules of at most 64 atoms take the wave form (form 0), larger ones the block form (1); shapemol_eval_sizes writes up to
 * n of (atoms of the wave form, atoms per molecule, elements, classes, edges per histogram, threads per workgroup) and
 * returns 6.  Limits, refused with a message before any kernel runs: 1..1024 atoms per molecule, n_elements 1..16, n_classes
 * 1..32, class slots inside the rule, 1..255 finite ascending edges per histogram, n_frames and n_mols 1..2^20.
 * shapemol_eval_check touches no device; it writes the form of every molecule to the optional h_forms (n_mols). */
typedef struct shapemol_eval_ctx shapemol_eval_ctx;
int shapemol_eval_sizes(int64_t *out, int32_t n);
int shapemol_eval_check(int64_t n_frames, int64_t n_mols, const int64_t *h_off, int32_t n_elements, int32_t n_classes,
                        const int32_t *h_class_slot, const double *h_cc_edges, int32_t n_cc, double cc_cut,
                        const double *h_all_edges, int32_t n_all, double all_cut, int32_t *h_forms);
int shapemol_eval_create(int device, shapemol_eval_ctx **out);
void shapemol_eval_destroy(shapemol_eval_ctx *ctx);
/* DEVICE inputs: d_pos (n_frames, N, 3) float32, d_classes (n_frames, N) int32, or int64 with classes_int64 != 0.  DEVICE
 * outputs, all written by the call: d_nr_bonds (n_frames, N) int32 the bond orders summed per atom; d_n_stable (n_frames,
 * n_mols) int32 the atoms whose sum s has valence >= s > 0 (hs != 0: valence == s); d_mol_stable (n_frames, n_mols) uint8
 * whether all atoms are; d_hist_cc (n_frames, n_cc + 1), d_hist_all (n_frames, n_all + 1) and d_class_counts (n_frames,
 * n_classes) int64.  The same in every run.  The call synchronises the stream.  Returns 0, or 1 with a message: a refused
 * call launches nothing; a class outside [0, n_classes) found on the device makes the outputs invalid.  Either way the
 * context stays usable.  A context serves one stream at a time. */
int shapemol_eval_run(shapemol_eval_ctx *ctx, int64_t n_frames, int64_t n_mols, const int64_t *h_off, const float *d_pos,
                      const void *d_classes, int32_t classes_int64, int32_t n_elements, const double *h_thresholds,
                      const double *h_allowed, int32_t carbon_slot, int32_t n_classes, const int32_t *h_class_slot,
                      const double *h_cc_edges, int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all,
                      double all_cut, int32_t hs, int32_t *d_nr_bonds, int32_t *d_n_stable, uint8_t *d_mol_stable,
                      int64_t *d_hist_cc, int64_t *d_hist_all, int64_t *d_class_counts, void *stream);
/* Tests only: fill the context's device workspace with `byte`. */
int shapemol_eval_debug_fill(shapemol_eval_ctx *ctx, int32_t byte, void *stream);

/* ---- Gaussian similarity of molecules: shape and electrostatic overlap, and the rigid overlay ------------------------------
 * What the reference's evaluation asks of shaep_utils.get_ROCS / shape_tanimoto / VAB_2nd_order and of espsim's
 * GetIntegralsViaGaussians / GaussInt / SimilarityMetric, plus a rigid overlay by this library's own rule where the reference
 * shells out to ShaEP.  Two packed sets of molecules, a and b: n_mols molecules back to back, HOST
 * h_off (n_mols + 1, starting at 0), DEVICE d_pos (N, 3) float64, HOST per-atom parameters h_u and h_v (N) float64.  HOST
 * h_pairs (n_pairs, 2) int64 names a molecule of a and one of b per pair, so N-to-1, 1-to-1 and all-pairs are one call.
 * mode 0 (shape): u = the Gaussian widths alpha, v = the prefactors p; one term per atom pair with s = alpha_i + alpha_j,
 * A = (pi^1.5 * (p_i * p_j)) / (s * sqrt(s)), B = (alpha_i * alpha_j) / s, w = 1.  mode 1 (esp): u = the charges w, v unused
 * (may be null); n_terms (1..16) terms with HOST h_term_a = A_k and h_term_b = B_k (GaussInt's b are -B_k).  An integral is
 * S_xy = sum_{i in x, j in y} w_i w_j sum_k A_k exp(-(B_k * r2)), r2 = (dx*dx + dy*dy) + dz*dz, float64 without FMA
 * contraction; the thread of atom i sums over j ascending, the threads' sums are added by a fixed binary tree: the same bits
 * in every run, no atomics.  metric 0: Tanimoto S_ab / ((S_aa + S_bb) - S_ab); metric 1: Carbo S_ab / sqrt(S_aa * S_bb).  A
 * denominator that equals 0 gives a NaN score and the pair's flag.
 * A pair whose molecules both have at most 64 atoms takes the wave form (form 0), any other the block form (1);
 * shapemol_sim_sizes writes up to n of (atoms of the wave form, atoms per molecule, terms, starts of an overlay, largest
 * iteration cap, pairs per call) and returns 6.  Limits, refused with a message before any kernel runs: 1..256 atoms per
 * molecule, 1..2^20 molecules per set, 1..2^22 pairs with indices inside their sets, finite parameters, widths > 0.
 * shapemol_sim_check touches no device; it writes the form of every pair to the optional h_forms (n_pairs). */
typedef struct shapemol_sim_ctx shapemol_sim_ctx;
int shapemol_sim_sizes(int64_t *out, int32_t n);
int shapemol_sim_check(int32_t mode, int64_t n_mols_a, const int64_t *h_off_a, const double *h_u_a, const double *h_v_a,
                       int64_t n_mols_b, const int64_t *h_off_b, const double *h_u_b, const double *h_v_b, int64_t n_pairs,
                       const int64_t *h_pairs, int32_t n_terms, const double *h_term_a, const double *h_term_b,
                       int32_t *h_forms);
int shapemol_sim_create(int device, shapemol_sim_ctx **out);
void shapemol_sim_destroy(shapemol_sim_ctx *ctx);
/* The fixed pose.  DEVICE outputs: d_out (n_pairs, 4) float64 = S_aa, S_bb, S_ab, score; d_flags (n_pairs) int32, 1 where the
 * denominator is 0.  The call synchronises the stream.  Returns 0, or 1 with a message; a refused call launches nothing and
 * the context stays usable.  A context serves one stream at a time. */
int shapemol_sim_score(shapemol_sim_ctx *ctx, int32_t mode, int32_t metric, int64_t n_mols_a, const int64_t *h_off_a,
                       const double *d_pos_a, const double *h_u_a, const double *h_v_a, int64_t n_mols_b,
                       const int64_t *h_off_b, const double *d_pos_b, const double *h_u_b, const double *h_v_b,
                       int64_t n_pairs, const int64_t *h_pairs, int32_t n_terms, const double *h_term_a,
                       const double *h_term_b, double *d_out, int32_t *d_flags, void *stream);
/* The overlay (shape mode): per pair, maximise S_ab over rigid motions of molecule a.  Starts 0..3: the proper rotations
 * Vb diag(1,1,1 | 1,-1,-1 | -1,1,-1 | -1,-1,1) Va^T that map a's principal frame onto b's with the centroids coincident (V:
 * eigenvectors of the unit-weight inertia tensor by cyclic Jacobi, ascending eigenvalues, third column = first x second);
 * start 4, with include_given, the pose as given.  From each start BFGS over (translation, rotation about a's centroid) with
 * the analytic gradient, steps of at most 0.5 (Angstrom, radian) per component, Armijo backtracking (1e-4, halving, at most
 * 30 times), until the largest gradient component is <= gtol * (S_aa + S_bb) / 2 (converged) or max_iter (0..10000)
 * iterations are used.  The start with the largest S_ab wins (ties: the lowest index).  The winner's motion is applied to the
 * coordinates of a as given, x' = ((R0 x + R1 y) + R2 z) + t per row, and the result is scored by the fixed-pose kernel; with
 * include_given the pose as given replaces it (start 4, identity, 0 iterations) when it scores higher, so the result is never
 * below it; the converged flag reported then is start 4's own if that start never left the pose as given, else 0.  A start
 * whose value or gradient is NaN (positions that are not finite) stops at once, not converged.  DEVICE outputs: d_out (n_pairs, 4) float64 = S_aa, S_bb, S_ab, Tanimoto; d_rot (n_pairs, 9) row-major and
 * d_trans (n_pairs, 3) float64; d_info (n_pairs, 4) int32 = winning start, its iterations, its converged flag, zero
 * denominator; d_aligned (optional, may be null): the moved copies of a, (sum over the pairs of their a's atoms, 3) float64
 * in pair order.  Synchronises the stream; errors as for shapemol_sim_score. */
int shapemol_sim_align(shapemol_sim_ctx *ctx, int64_t n_mols_a, const int64_t *h_off_a, const double *d_pos_a,
                       const double *h_alpha_a, const double *h_p_a, int64_t n_mols_b, const int64_t *h_off_b,
                       const double *d_pos_b, const double *h_alpha_b, const double *h_p_b, int64_t n_pairs,
                       const int64_t *h_pairs, int32_t include_given, int32_t max_iter, double gtol, double *d_out,
                       double *d_rot, double *d_trans, int32_t *d_info, double *d_aligned, void *stream);
/* Tests only: fill the context's device workspaces with `byte`. */
int shapemol_sim_debug_fill(shapemol_sim_ctx *ctx, int32_t byte, void *stream);

/* ---- bond graphs of sampled molecules: bonds, fragments, rings, bond lengths ------------------------------------------------
 * What the reference's evaluation script needs once it knows which atoms are bonded, with the bonds
 * decided by THIS library's rule, the thresholds of shapemol_eval_* above (a pair is a bond when its order is > 0), not by a
 * chemistry toolkit's perception.  Inputs as for shapemol_eval_run, plus h_bl_edges (n_bl): the bond-length bin edges.
 * Molecules of at most 64 atoms take the wave form (0), molecules of 65..256 atoms the block form (1); shapemol_graph_sizes
 * writes up to n of (atoms of the wave form, atoms per molecule, elements, classes, edges per histogram, threads per
 * workgroup, bits of ring_sizes) and returns 7.  Limits, refused with a message that names the molecule or argument before
 * any kernel runs: 1..256 atoms per molecule, n_elements 1..16, n_classes 1..32, class slots inside the rule, 1..255 finite
 * ascending edges per histogram, n_frames and n_mols 1..2^20.  The bonds of a call are counted on the device; a call with
 * 2^31 or more is refused after the count and before anything is written.  shapemol_graph_check touches no device; it
 * writes the form of every molecule to the optional h_forms (n_mols). */
typedef struct shapemol_graph_ctx shapemol_graph_ctx;
int shapemol_graph_sizes(int64_t *out, int32_t n);
int shapemol_graph_check(int64_t n_frames, int64_t n_mols, const int64_t *h_off, int32_t n_elements, int32_t n_classes,
                         const int32_t *h_class_slot, const double *h_cc_edges, int32_t n_cc, double cc_cut,
                         const double *h_all_edges, int32_t n_all, double all_cut, const double *h_bl_edges, int32_t n_bl,
                         int32_t *h_forms);
int shapemol_graph_create(int device, shapemol_graph_ctx **out);
void shapemol_graph_destroy(shapemol_graph_ctx *ctx);
/* Count pass, scan, fill pass with the rings.  DEVICE outputs, all int32 and all written by the call: d_nr_bonds, d_degree,
 * d_frag, d_ring_atom (n_frames, N) = the bond orders summed per atom (shapemol_eval_run's d_nr_bonds), the bonds per atom,
 * the smallest atom index (within the frame) of the atom's fragment, the smallest ring through one of the atom's bonds (0:
 * none); d_mol (n_frames, n_mols, 6) = bonds, fragments, atoms of the largest fragment, complete (one fragment), cyclomatic
 * number bonds - atoms + fragments, ring_sizes (bit s, 3 <= s <= 30: some bond's shortest cycle has s bonds; bit 31: more).
 * int64 counters per frame, zeroed by the call: d_hist_bl (n_frames, 2, E (E + 1) / 2, 3, n_bl + 1) bond lengths over all
 * molecules | over complete ones, per pair of element slots a <= b (row-major upper triangle), order 1..3 and bin
 * np.searchsorted(edges, d, 'left'); d_hist_cc, d_hist_all, d_class_counts as for shapemol_eval_run but over complete
 * molecules only; d_frame_counts (n_frames, 33) = complete molecules, then molecules whose ring_sizes has bit 0..31.
 * *h_total = the bonds of the call.  The bond list stays in the context until its next run: shapemol_graph_bonds copies the
 * first n_items scalars of the offsets (which = 0, int64, n_frames * n_mols + 1), the bonds (1, int32, (total, 3) = atom i,
 * atom j > i, order, sorted by frame, molecule, i, j; atoms indexed within the frame) or their rings (2, int32, total: bonds
 * in the shortest cycle through the bond, 0 for a bridge) to dst, HOST or DEVICE.  The same in every run.  Both calls
 * synchronise the stream (the run twice: the host reads the bond total between the passes).  Return 0, or 1 with a message:
 * a refused call launches nothing; a class outside [0, n_classes) found on the device makes the outputs invalid.  Either way
 * the context stays usable.  A context serves one stream at a time. */
int shapemol_graph_run(shapemol_graph_ctx *ctx, int64_t n_frames, int64_t n_mols, const int64_t *h_off, const float *d_pos,
                       const void *d_classes, int32_t classes_int64, int32_t n_elements, const double *h_thresholds,
                       int32_t carbon_slot, int32_t n_classes, const int32_t *h_class_slot, const double *h_cc_edges,
                       int32_t n_cc, double cc_cut, const double *h_all_edges, int32_t n_all, double all_cut,
                       const double *h_bl_edges, int32_t n_bl, int32_t *d_nr_bonds, int32_t *d_degree, int32_t *d_frag,
                       int32_t *d_ring_atom, int32_t *d_mol, int64_t *d_hist_bl, int64_t *d_hist_cc, int64_t *d_hist_all,
                       int64_t *d_class_counts, int64_t *d_frame_counts, int64_t *h_total, void *stream);
int shapemol_graph_bonds(shapemol_graph_ctx *ctx, int32_t which, void *dst, int64_t n_items, void *stream);
/* Tests only: fill the context's device workspaces with `byte`; the last run's bond list is gone afterwards. */
int shapemol_graph_debug_fill(shapemol_graph_ctx *ctx, int32_t byte, void *stream);

/* Per-kernel launch-time accounting with HIP events on the launch stream (bench only).
 * shapemol_profile_begin() arms it for the following _score/_sample calls (forces eager launches);
 * shapemol_profile_end() synchronises and writes, for each of up to `cap` kernel classes,
 * name / total milliseconds / launch count.  Returns the number of classes. */
int shapemol_profile_begin(shapemol_ctx *ctx);
int shapemol_profile_end(shapemol_ctx *ctx, char (*names)[32], double *total_ms, int64_t *launches, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SHAPEMOL_HIP_H */
