/*
 * ls2fm.h -- C ABI of libls2fm_hip.so: the MI355X (gfx950) implementation of Level-S2fM's
 * SDF ray-marching / volumetric-rendering hot path.
 *
 * Every entry point replaces something the reference reaches through a native extension or
 * through PyTorch device code on that path; the replaced interface is cited per function
 * (file:line relative to the reference tree).  The reference-side bindings a maintainer
 * would add are shown in INTEGRATION.md.
 *
 * Conventions (all functions)
 *   - plain C types only: raw DEVICE pointers, sizes, small by-value descriptor structs that
 *     live in HOST memory; no torch types
 *   - all tensors are contiguous, row-major; float = IEEE fp32, indices are uint32/int32/int64
 *   - the caller owns every buffer (inputs, outputs, gradient accumulators, workspace); the
 *     library never allocates device memory and keeps no global state
 *   - asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream); buffers must stay alive until the stream reaches the end of the call
 *   - gradient outputs documented as "accumulate" are added to with atomics and must be
 *     zeroed (or hold a running sum) by the caller; all others are overwritten
 *   - return value: 0 on success, a negative ls2fm_status otherwise (nothing is enqueued on
 *     LS2FM_ERR_INVALID_ARGUMENT / LS2FM_ERR_UNSUPPORTED); thread-safe for distinct streams
 */
#ifndef LS2FM_H
#define LS2FM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LS2FM_ABI_VERSION 13
#define LS2FM_MAX_LEVELS 16
#define LS2FM_HIDDEN 64        /* SDF.arch.layers = [null, 64, 16]  (options/LevelS2fM.yaml:14) */
#define LS2FM_FEAT 16
#define LS2FM_VIEW_ENC 27      /* Fourier view embedding, 4 octaves (models/base.py:143-151) */

typedef enum ls2fm_status {
    LS2FM_OK = 0,
    LS2FM_ERR_INVALID_ARGUMENT = -1,
    LS2FM_ERR_UNSUPPORTED = -2,
    LS2FM_ERR_LAUNCH = -3,
    LS2FM_ERR_WORKSPACE = -4,
    LS2FM_ERR_STARVED = -5     /* an EARLIER asynchronous call reported a starved in-launch hand-off (ls2fm_async_error) */
} ls2fm_status;

/* Geometry of one multiresolution hash grid (tcnn Grid/Hash/Linear, n_features_per_level = 2).
 * Built on the host (level-s2fm_official_amd/ls2fm/hashgrid.py) exactly as tcnn's constructor
 * does (grid_scale / grid_resolution / offset table); replaces the `encoding_config` dict the
 * reference hands to tinycudann.Encoding (models/base.py:17, :130-139). */
typedef struct ls2fm_grid_desc {
    int32_t n_levels;                         /* <= LS2FM_MAX_LEVELS */
    int32_t n_features;                       /* must be 2 */
    float scale[LS2FM_MAX_LEVELS];            /* grid_scale(level) */
    uint32_t resolution[LS2FM_MAX_LEVELS];    /* ceil(scale) + 1 */
    uint32_t size[LS2FM_MAX_LEVELS];          /* entries in the level */
    uint32_t offset[LS2FM_MAX_LEVELS + 1];    /* first entry of the level (in entries, not floats) */
    uint32_t hashed[LS2FM_MAX_LEVELS];        /* 1: coherent prime hash, 0: dense stride walk */
} ls2fm_grid_desc;

/* Scene / field constants the path reads from `opt` (SURVEY.md section 5 "config / flags"). */
typedef struct ls2fm_field_desc {
    float bound_min[3];      /* opt.data.bound_min */
    float bound_max[3];      /* opt.data.bound_max */
    float rescale;           /* opt.SDF.VolSDF.rescale        (models/base.py:38-40) */
    float scale_mlp;         /* opt.SDF.NN_Init.scale_mlp: sdf = +-f0 / scale_mlp (true division) */
    int32_t inside;          /* opt.data.inside: sign of the sdf (models/SDF.py:66-71) */
    int32_t bg_sdf;          /* opt.data.inside && opt.data.bg_sdf: sdf = min(sdf, bg_rad - |p|) */
    float bg_rad;
    float bgcolor[3];        /* models/Renderer.py:25-31 */
    int32_t n_samples;       /* opt.SDF.VolSDF.sample_intvs */
    int32_t dual_field;      /* opt.Ablate_config.dual_field */
} ls2fm_field_desc;

/* One weight-normed linear layer as the reference stores it (legacy torch weight_norm, dim 0):
 * W[o][i] = g[o] * v[o][i] / ||v[o]||,  models/base.py:200, :241; state_dict keys App. E. */
typedef struct ls2fm_linear {
    const float* weight_v;   /* [out][in] */
    const float* weight_g;   /* [out]     */
    const float* bias;       /* [out]     */
} ls2fm_linear;

typedef struct ls2fm_linear_grad {      /* same shapes; overwritten */
    float* weight_v;
    float* weight_g;
    float* bias;
} ls2fm_linear_grad;

/* All learnable state of the path (device pointers into the nn.Parameters). */
typedef struct ls2fm_params {
    const float* sdf_table;             /* SDF.embed_fn.embedder_obj.params        [n_params] */
    ls2fm_linear sdf_mlp[2];            /* SDF.SDF_MLP.mlp.{0,1}: (3+2L)->64->17   */
    const float* beta;                  /* SDF.beta [1] (log-space parameter, SDF.py:28-32) */
    float beta_speed;                   /* opt.SDF.VolSDF.beta_speed */
    const float* rad_table;             /* RadF.embed_fn.embedder_obj.params (dual field) or NULL */
    ls2fm_linear geo_mlp[2];            /* RadF.Geo_enc.mlp.{0,1} (dual field) */
    ls2fm_linear rad_mlp[3];            /* RadF.Rad_dec.mlp_radiance.{0,1,2}: (49|65)->64->64->3 */
    const float* dual_table;            /* optional (dual field): both tables entry-interleaved, [n_entries][4] =
                                           {sdf f0, sdf f1, rad f0, rad f1}, as ls2fm_interleave_tables writes it and in
                                           sync with sdf_table / rad_table; NULL: gather from the two tables */
} ls2fm_params;

typedef struct ls2fm_param_grads {      /* mirrors ls2fm_params */
    float* sdf_table;                   /* overwritten in full (LDS-slab scatter, no atomics) */
    ls2fm_linear_grad sdf_mlp[2];
    float* beta;                        /* [1] overwritten */
    float* rad_table;                   /* overwritten in full */
    ls2fm_linear_grad geo_mlp[2];
    ls2fm_linear_grad rad_mlp[3];
} ls2fm_param_grads;

int ls2fm_abi_version(void);
const char* ls2fm_status_string(int status);
/* Sticky error word of the ASYNCHRONOUS part of earlier calls (0 = none).  The render backward hands partial sums between
 * workgroups of ONE launch (weight-gradient reduction rows / finalize tasks behind their producers); consumers poll with a bound, and
 * one that gives up (producers starved of execution slots: a device cut down by a CU mask, a foreign kernel that never ends) poisons
 * its outputs with NaN AND sets this word (1) in host-visible memory -- no synchronisation is needed to read it, and every later
 * ls2fm_render_bwd returns LS2FM_ERR_STARVED until it is cleared.  clear != 0: reset after reading.  No reference counterpart
 * (autograd's kernels have no in-launch hand-offs). */
int ls2fm_async_error(int clear);

/* ---------------------------------------------------------------------------------------------
 * Ray / AABB slab test.
 * Replaces: vren.ray_aabb_intersect as bound by utils/custom_functions.py:28-31
 *           (called from models/Renderer.py:178-179 and models/SDF.py:120-121).
 * rays_o, rays_d [n_rays,3] (directions NOT normalised); center, half_size [n_voxels,3].
 * Outputs: hits_cnt int32[n_rays]; hits_t float[n_rays,max_hits,2] (near clamped to >= 0; -1,-1 in
 * unused slots); hits_voxel_idx int64[n_rays,max_hits] (-1 in unused slots); slots sorted by near t.
 */
int ls2fm_ray_aabb_intersect(const float* rays_o, const float* rays_d, const float* center,
                             const float* half_size, int64_t n_rays, int32_t n_voxels, int32_t max_hits,
                             int32_t* hits_cnt, float* hits_t, int64_t* hits_voxel_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multiresolution hash-grid encoding (fp32), forward / backward / double backward.
 * Replaces: tinycudann.Encoding(Grid, Hash, Linear) -- constructor models/base.py:17, forward
 *           models/base.py:37; its backward is reached through loss.backward() and its double
 *           backward through SDF.gradient's create_graph=True (models/SDF.py:102-114).
 * x [n,3] is the NORMALISED position the reference feeds ((p-bmin)/(bmax-bmin), base.py:35); no
 * clamping.  y [n, L*2] is level-major ([l*2+f]).  dy_dx [n, L*2, 3] optional (NULL to skip).
 */
int ls2fm_grid_encode_fwd(const ls2fm_grid_desc* grid, const float* x, const float* table, int64_t n,
                          float* y, float* dy_dx, void* stream);

/* dtable (accumulate, NULL to skip) += scatter of dy;  dx [n,3] (overwritten, NULL to skip). */
int ls2fm_grid_encode_bwd(const ls2fm_grid_desc* grid, const float* x, const float* table, const float* dy,
                          int64_t n, float* dtable, float* dx, void* stream);

/* Backward of the map (dy, table, x) -> dx of ls2fm_grid_encode_bwd, given ddx = dL/d(dx) [n,3]:
 *   d_dy [n,L*2] (overwritten), dtable (accumulate), dx2 [n,3] (overwritten; mixed second partials).
 * Any output may be NULL. */
int ls2fm_grid_encode_bwd_bwd(const ls2fm_grid_desc* grid, const float* x, const float* table,
                              const float* dy, const float* ddx, int64_t n, float* d_dy, float* dtable,
                              float* dx2, void* stream);

/* Debug / parity: the 8 level-local corner indices per (point, level): out uint32[n, L, 8]. */
int ls2fm_grid_indices(const ls2fm_grid_desc* grid, const float* x, int64_t n, uint32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused SDF evaluation without autograd: hash encode -> 35->64 softplus(100) -> 64->17, sign /
 * scale_mlp, optional analytic normal d sdf / d p.
 * Replaces: SDF.infer_sdf (models/SDF.py:55-78) in its no-grad uses (sphere-tracing inner loop
 *           SDF.py:185-196, mesh sweeps utils/util.py:426-428) and SDF.gradient (SDF.py:102-114)
 *           when no graph is needed.
 * p [n,3] world positions.  sdf [n]; feat [n,17] or NULL; normal [n,3] or NULL.
 * workspace: ls2fm_sdf_eval_workspace_bytes() bytes.
 */
int64_t ls2fm_sdf_eval_workspace_bytes(void);
int ls2fm_sdf_eval(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                   const float* p, int64_t n, float* sdf, float* feat, float* normal, void* workspace,
                   void* stream);

/* No-grad SDF sweep over an n_side^3 lattice generated on the device: sdf[i] = infer_sdf(point(first + i)), i < count.
 * Replaces: the batchify loop of extract_mesh (utils/util.py:411-424: 16 k-point chunks, each a host->device copy,
 * infer_sdf, device->host copy) and its host-side numpy lattice (util.py:399-409).
 * With idx = first + i:  ref_indexing != 0: column c of the point = fl32(f_c * step[c] + origin[c]) in fp64 with
 * f = (fmod(idx/N/N, N), fmod(idx/N, N), idx mod N) under TRUE division -- exactly the reference's arithmetic (its first
 * two index columns are fractional); ref_indexing == 0: f = integer lattice indices (idx div N^2, idx div N mod N,
 * idx mod N).  workspace: ls2fm_sdf_eval_workspace_bytes().
 */
int ls2fm_sdf_volume(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                     int64_t n_side, int64_t first, int64_t count, int32_t ref_indexing, const double* step,
                     const double* origin, float* sdf, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Marching cubes over a dense volume: the mesh of the level set {v = level}.
 * Replaces: skimage.measure.marching_cubes as called by convert_sigma_samples_to_ply (utils/util.py:345), reached from
 *           extract_mesh (util.py:392-425) on the volume of ls2fm_sdf_volume.
 * vol [nx,ny,nz] fp32, row-major (axis 2 fastest).  Corner values v < level (strict; a NaN is not) are BELOW; an edge
 * crosses iff exactly one end is below.  Case table generated from one face rule (csrc/mc_tables.h, tools/gen_mc_tables.py):
 * shared faces get the same segments, so the mesh has no cracks; an ambiguous face cuts each below corner off on its own
 * (simpler than skimage's Lewiner tables: topology in ambiguous cells may differ).  Triangle normals (right-hand rule) point
 * to increasing values (outward for an SDF).
 * verts float [n_verts,3], one per crossing lattice edge, ordered by (lower end's linear index, axis 0 < 1 < 2):
 *   t = (level - v0) / (v1 - v0),  pos[a] = (idx[a] + (a == axis ? t : 0)) * spacing[a] + origin[a]  (fp32, each op rounded);
 * faces int32 [n_faces,3] vertex ids, ordered by (cell linear index, table order).  Output is deterministic.
 * Refused (LS2FM_ERR_INVALID_ARGUMENT, nothing enqueued): any side < 2, or 3 nx ny nz >= 2^31 (vertex ids are int32).
 * ls2fm_marching_cubes_workspace_bytes: bytes of workspace (~5 per point), or < 0 for refused sizes.
 * ls2fm_marching_cubes_count: counts int64 [2] (device) = n_verts, n_faces; fills the workspace for the emit call.
 * ls2fm_marching_cubes_emit: after count, with the same volume, level and workspace; verts / faces hold at least the counted
 * rows (either may be NULL when its count is 0).  spacing, origin: 3 floats each in HOST memory.
 */
int64_t ls2fm_marching_cubes_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int ls2fm_marching_cubes_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace,
                               int64_t* counts, void* stream);
int ls2fm_marching_cubes_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, const float* spacing,
                              const float* origin, void* workspace, float* verts, int32_t* faces, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh components and the largest component by area (new, ABI 13).
 * Replaces: trimesh.Trimesh.split(only_watertight=False), argmax over the components' `area` and the submesh it returns, as
 *           get_surface_high_res_mesh calls them (utils/plots.py:163-166).
 * verts fp32 [n_verts,3], faces int32 [n_faces,3], DEVICE.  Every index lies in [0, n_verts): the caller guarantees it (the
 * library does not check; ls2fm.mesh checks with one device reduction before the call).
 * Components: two faces are in one component when a chain of faces, each consecutive pair sharing a vertex INDEX, links them
 * (trimesh joins through shared edges; on ls2fm_marching_cubes meshes the two agree).  The label of a vertex is the smallest
 * vertex index of its component; a vertex no face uses is a component of its own.  Labels do not depend on the order of the
 * unions: they are deterministic by definition.
 * Area of a face: 0.5 |(b - a) x (c - a)| in double from the fp32 corners; of a component: the sum over its faces, formed in
 * 64-bit fixed point (2^-s units, s from the largest face area and n_faces, so the total stays below 2^63): the sum does not
 * depend on the order of the faces, two components with the same faces tie exactly, and every call gives the same bits.
 * Largest component: the largest area; on a tie, the component that holds the lowest-numbered face (what np.argmax over
 * trimesh's split list, ordered by lowest face, picks).  Extraction keeps its faces in their order and the vertices they use
 * in index order, the faces renumbered to match (Trimesh.submesh).  Output is identical from call to call.
 * ls2fm_mesh_components: labels int32 [n_verts].  n_faces = 0 writes labels[v] = v (one launch); n_verts = 0 enqueues nothing.
 * ls2fm_mesh_components_workspace_bytes: workspace of the two calls below (~20 bytes per vertex), or < 0 for refused sizes.
 * ls2fm_mesh_largest_component_count: counts int64 [2] (device) = kept vertices, kept faces; areas double [n_verts] or NULL:
 *   areas[l] = the area of the component labelled l, 0 where l is no label.  Fills the workspace for the emit call.
 * ls2fm_mesh_largest_component_emit: after count, with the same mesh and workspace; out_verts [counts[0],3] fp32, out_faces
 *   [counts[1],3] int32.
 * n_faces = 0: the result is empty; nothing is enqueued and counts are not written.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL buffer, a negative count, n_verts >= 2^31,
 * n_faces >= 2^31 or faces without vertices; LS2FM_ERR_WORKSPACE for a NULL workspace or one below the queried size.
 */
int64_t ls2fm_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces);
int ls2fm_mesh_components(const int32_t* faces, int64_t n_verts, int64_t n_faces, int32_t* labels, void* stream);
int ls2fm_mesh_largest_component_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                       void* workspace, int64_t workspace_bytes, int64_t* counts, double* areas, void* stream);
int ls2fm_mesh_largest_component_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                      void* workspace, int64_t workspace_bytes, float* out_verts, int32_t* out_faces,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Point queries WITH a graph: backward of  p -> (sdf, the 17 MLP outputs, the analytic normal d sdf / d p)  for n free points.
 * Replaces: what loss.backward() traverses for SDF.infer_sdf with parameters requiring grad (models/SDF.py:55-78),
 * SDF.gradient (SDF.py:102-114: autograd.grad(create_graph=True) -- callers take norms of it inside losses:
 * pipelines/Registration.py:202,259-261, BA.py:123-125) and SDF.get_surface_pts (SDF.py:95-100): tcnn's backward and
 * double-backward kernels plus the torch Linear / Softplus / weight_norm backward nodes and their double backward.
 * The forward is ls2fm_sdf_eval (same values; nothing is kept from it).  Upstreams (any may be NULL = zeros, not all):
 * d_sdf [n], d_feat [n,17] (raw MLP outputs; column 0 is f0, sdf = +-f0 / scale_mlp), d_normal [n,3].
 * grads: sdf_table (overwritten in full), sdf_mlp[0..1] (weight_v / weight_g / bias, overwritten); other members ignored.
 * d_p [n,3] (overwritten) or NULL.  No background-sphere min (LS2FM_ERR_UNSUPPORTED: general composed form).
 * workspace: ls2fm_sdf_points_workspace_bytes(...) bytes, scratch for this call only.
 */
int64_t ls2fm_sdf_points_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, int64_t n_points);
int ls2fm_sdf_points_bwd(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                         const float* p, int64_t n, const float* d_sdf, const float* d_feat, const float* d_normal,
                         const ls2fm_param_grads* grads, float* d_p, void* workspace, void* stream);
/* The same, as a SECOND gradient producer of a backward pass: the parameter gradients are ADDED to what `grads` already holds
 * (written earlier on the same stream, e.g. by ls2fm_render_bwd) -- the table through the scatter's add mode (nothing is zeroed,
 * slabs without items are not touched), the MLP tensors through the weight-norm backward's.  d_p is overwritten as above.  What
 * autograd otherwise does with two dense 50 MB table gradients and seven small tensors per extra node: a sum kernel each. */
int ls2fm_sdf_points_bwd_add(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                             const float* p, int64_t n, const float* d_sdf, const float* d_feat, const float* d_normal,
                             const ls2fm_param_grads* grads, float* d_p, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused volumetric rendering, forward.
 * Replaces: Renderer.forward (models/Renderer.py:51-116) and everything it calls: ray/AABB near-far
 * (Renderer.py:178), uniform mid-point sampling (Renderer.py:118-127), p = c + d t (utils/camera.py:
 * 262-266), SDF.infer_sdf + SDF.gradient (SDF.py:55-78, 102-114), RadF.Geometry_feat / infer_embed_v /
 * infer_app (RadF.py:66-86), SDF.sdf_to_sigma (SDF.py:84-87), Renderer.composite (Renderer.py:33-49)
 * and the background / depth / normal epilogue (Renderer.py:89-107).
 * center, ray [n_rays,3].  Outputs: rgb [n_rays,3], sdfs_volume [n_rays,N], normals [n_rays,N,3],
 * depth_mlp [n_rays], normal_mlp [n_rays,3].
 * workspace: ls2fm_render_workspace_bytes(...) bytes; its contents are consumed by ls2fm_render_bwd
 * for the same inputs, so it must be kept untouched between the two calls (ls2fm_render_bwd may run more than once on it).
 * The hash-table gradient outputs of ls2fm_render_bwd must be 16-byte aligned (float4 stores).
 */
#define LS2FM_MAX_RENDER_POINTS (1 << 23)   /* n_rays * n_samples per call (32-bit element / byte offsets and item counts
                                               inside); more: LS2FM_ERR_UNSUPPORTED from the size query, ls2fm_render_fwd
                                               and ls2fm_render_bwd -- split the rays over several calls */
int64_t ls2fm_render_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, int64_t n_rays);
/* Dual field, optional: write both hash tables (same geometry, [n_entries][2] each) entry-interleaved into
 * dual_table [n_entries][4] for ls2fm_params.dual_table.  The forward then gathers ONE 16-byte entry per corner for both
 * encodings instead of two 8-byte ones (the gathers are request-rate bound).  The caller owns the
 * buffer and refreshes it whenever either table changed (the host side keys it on the parameters' version counters). */
int ls2fm_interleave_tables(const float* sdf_table, const float* rad_table, int64_t n_entries, float* dual_table,
                            void* stream);
/* Optional extras of one render call (HOST struct; NULL = a plain render that a backward may follow).
 *   inference_only  forward: non-zero = no ls2fm_render_bwd will follow on this workspace.  Otherwise the forward's gather
 *                   pass also counts the items of the backward's table-gradient scatter (the corner cells are known there
 *                   anyway) and scans them beside shade_fwd, so the backward starts its scatter without a counting pass.
 *   n_level_groups, group_events   see the struct.
 *   loss            the loss head of the stage loops evaluated INSIDE the render (SURVEY.md section 8f row 1 "fuse as an
 *                   epilogue of the render kernel"; replaces pipelines/Camera.py:515-537 + BA.py:206-218 exactly as
 *                   ls2fm_loss_head_fwd/bwd below do, same tensors, same `terms` / `sums` layout): the forward's last kernel
 *                   forms the per-ray partial sums while rgb / normals / depth are still in registers and a one-workgroup
 *                   reduction writes `terms` and `sums`; the backward forms d rgb / d normals / d depth per sample from
 *                   `sums` (the counts), `weights` and the scalar upstreams `d_terms` / `d_total` in its first kernel -- no
 *                   [n_rays, N, 3] gradient tensor, no loss kernels between forward and backward.  Explicit upstreams
 *                   (d_rgb ... of ls2fm_render_bwd) are added on top.  A sharded run may all-reduce `sums` between the two
 *                   calls (and refresh `terms` with ls2fm_loss_terms_from_sums) for world-size-invariant means.
 */
typedef struct ls2fm_loss_spec {
    const float* rgb_gt;          /* [n_rays,3] */
    const float* depth_ref;       /* [n_rays] sphere-traced depth, or NULL = no depth-consistency term */
    const uint8_t* mask_eik;      /* [n_rays] or NULL = every ray: rays whose samples enter the eikonal mean */
    const uint8_t* mask_dc;       /* [n_rays] or NULL: mask_finish */
    const uint8_t* mask_mse;      /* [n_rays] or NULL: mask_bg */
    const float* weights;         /* DEVICE float[3] = 10^w of (rgb, eikonal, DC) */
    float* terms;                 /* DEVICE float[8]: forward output (layout of ls2fm_loss_head_fwd) */
    double* sums;                 /* DEVICE double[8]: forward output, backward input */
    const float* d_terms;         /* backward: DEVICE float[5] upstream of terms[0..4], or NULL = zeros */
    const float* d_total;         /* backward: DEVICE float[1] additional upstream of the weighted total, or NULL */
    float* d_depth_ref;           /* backward output: [n_rays] gradient w.r.t. depth_ref (overwritten), or NULL */
    uint32_t flags;               /* LS2FM_LOSS_*_FROM_GT */
    uint32_t count_scale;         /* ABI 9 (in the struct's former padding: size and offsets unchanged).  > 1: every COUNT of `sums` is
                                     multiplied by it in the forward's reduction -- a data-parallel run whose ranks hold the same number
                                     of rays and no masks divides by the GLOBAL counts without a collective or a kernel between forward and
                                     backward (ls2fm.dist "uniform"); 0 / 1: the local counts */
} ls2fm_loss_spec;
/* mask_eik / mask_mse := CameraSet.render's mask_bg, 0.05 < mean(rgb_gt[r]) < 0.95 (Camera.py:515), evaluated in the kernels
 * from rgb_gt; the pointer of the same name is ignored.  With these the loss head's only inputs that come out of a sphere
 * tracing are depth_ref and mask_dc (see ls2fm_render_opts.loss_inputs_ready). */
#define LS2FM_LOSS_EIK_FROM_GT 1u
#define LS2FM_LOSS_MSE_FROM_GT 2u

/* The backward of the sphere tracing that produced a render's depth_ref, run BY ls2fm_render_bwd and merged into its own
 * chains.  On an internal stream of its own, forked behind the call's first kernel (which writes d_depth_ref): the masked
 * upstream of the track points (ls2fm_trace_depth_bwd) and the front stages of ls2fm_sdf_points_bwd over them (gather pass,
 * per-point backward, scans, payload sort).  Then the per-point rows are contracted by the render's own SDF weight-gradient
 * kernel as extra tiles, and the points' table gradient is added into the render's sdf_table gradient behind its scatter: the
 * render's `grads` come out as the SUM of both producers -- no second set of gradient tensors, no sum kernel.  Replaces what
 * autograd does for Camera.py:506-523's d_consistent term through SDF.sphere_tracing's differentiable tail (SDF.py:201-214): a
 * second backward chain and seven accumulation kernels.  Not combined with n_level_groups > 1 (LS2FM_ERR_UNSUPPORTED). */
typedef struct ls2fm_depth_backward {
    const float* points;          /* [n_rays * k_max, 3] the tracing's track points (ls2fm_sphere_trace) */
    const int32_t* trips;         /* DEVICE int32[1] */
    const uint8_t* gate;          /* [n_rays] from ls2fm_trace_depth_fwd */
    int32_t k_max;
    float* d_sdf;                 /* scratch [n_rays * k_max] */
    void* workspace;              /* ls2fm_sdf_points_workspace_bytes(field, grid, n_rays * k_max) bytes */
} ls2fm_depth_backward;

#define LS2FM_MAX_LEVEL_GROUPS 4
typedef struct ls2fm_render_opts {
    int32_t inference_only;
    const ls2fm_loss_spec* loss;  /* NULL: no fused loss head */
    /* backward, multi-GPU runs: scatter the table gradients in n_level_groups (2..4) groups of consecutive levels -- group g
     * holds levels [L g / n, L (g + 1) / n) -- and record group_events[g] (hipEvent_t, may be NULL) on `stream` once group g's
     * slices of the gradient tables are final, so that their all-reduce overlaps with the scatter of the later groups.
     * 0 / 1: one pass, no events. */
    int32_t n_level_groups;
    void* group_events[LS2FM_MAX_LEVEL_GROUPS];
    /* forward with a loss head: hipEvent_t (or NULL) after which depth_ref and mask_dc -- the outputs of the sphere tracing of
     * the same rays -- are final (mask_eik / mask_mse, when given as pointers, must be final in stream order at the call).  The
     * forward waits for it on `stream` only in front of the kernel that reads them, the loss reduction BEHIND its gather pass
     * and its shading kernel (which leaves the ray's depth for the reduction to form the depth-consistency term): a caller that
     * traces on another stream overlaps the whole tracing chain (latency bound, few workgroups) with both. */
    void* loss_inputs_ready;
    /* backward with a loss head: hipEvent_t (or NULL) RECORDED on `stream` as soon as the backward's first kernel is enqueued --
     * from then on d_depth_ref (the gradient w.r.t. the traced depth) is final in stream order.  A caller whose depth came from a
     * differentiable sphere tracing starts that tracing's own backward on another stream behind this event, i.e. beside the
     * table scatter and the weight-gradient chain of this call instead of behind them. */
    void* depth_grad_ready;
    /* backward with a loss head whose d_depth_ref is set: also run the tracing's backward (see ls2fm_depth_backward), or NULL */
    const ls2fm_depth_backward* depth_bwd;
} ls2fm_render_opts;

int ls2fm_render_fwd(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid,
                     const ls2fm_grid_desc* rad_grid, const ls2fm_params* params, const float* center,
                     const float* ray, int64_t n_rays, float* rgb, float* sdfs_volume, float* normals,
                     float* depth_mlp, float* normal_mlp, void* workspace, const ls2fm_render_opts* opts, void* stream);

/* Fused backward of ls2fm_render_fwd, including the analytic double backward of the normal path
 * (normals feed the radiance decoder, normal_mlp and the eikonal loss).
 * Upstream gradients (any may be NULL = zero): d_rgb [n_rays,3], d_sdfs_volume [n_rays,N],
 * d_normals [n_rays,N,3], d_depth_mlp [n_rays], d_normal_mlp [n_rays,3].
 * Parameter gradients go to `grads` in the reference's own parametrisation (weight_v/weight_g/bias,
 * beta).  d_center / d_ray [n_rays,3] (overwritten) may be NULL; when requested they carry the full
 * pose gradient (near/far are constants, exactly as in the reference: SURVEY.md 8a row a1).
 */
int ls2fm_render_bwd(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid,
                     const ls2fm_grid_desc* rad_grid, const ls2fm_params* params, const float* center,
                     const float* ray, int64_t n_rays, const float* d_rgb, const float* d_sdfs_volume,
                     const float* d_normals, const float* d_depth_mlp, const float* d_normal_mlp,
                     const ls2fm_param_grads* grads, float* d_center, float* d_ray, void* workspace,
                     const ls2fm_render_opts* opts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward-only rendering of whole images (new, ABI 12).
 * Replaces: Camera.render_img_by_slices (pipelines/Camera.py:274-311): get_center_and_ray for every pixel, then Renderer.forward
 * over rand_rays slices and a concatenation.
 * Every pixel's outputs are, bit for bit, what ls2fm_render_fwd returns for its ray -- the ray ls2fm_camera_rays forms for
 * poses and pix = 0 .. H*W-1 with width W (centres x + 0.5, y + 0.5):
 *   rgb [n_views,H*W,3] (background added), depth [n_views,H*W] (depth_mlp), normal [n_views,H*W,3] (normal_mlp),
 *   opacity [n_views,H*W] or NULL (the sum of the composite's weights, prob.sum: Renderer.py:89-107).  Row-major pixels.
 * poses [n_views,3,4] world-to-camera (DEVICE: read at run time, so a captured call follows poses updated in place);
 * kinv_host: the 3 x 3 K^-1 as 9 HOST floats (as ls2fm_camera_rays).
 * workspace: ls2fm_render_image_workspace_bytes(...) bytes: it depends on the field and the grids only, one call renders any
 * image size and any number of views (the rays are walked in chunks inside; LS2FM_MAX_RENDER_POINTS does not apply).  No
 * allocation, no host synchronisation, no stream fork: capturable.
 * Refusals (before any device work): LS2FM_ERR_UNSUPPORTED for bg_sdf, dual grids of different geometry and more than 512
 * samples per ray; LS2FM_ERR_INVALID_ARGUMENT for null inputs / outputs or non-positive sizes; LS2FM_ERR_WORKSPACE for a null
 * workspace.  No gradients (the reference renders images under no_grad).
 */
int64_t ls2fm_render_image_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid,
                                           const ls2fm_grid_desc* rad_grid);
int ls2fm_render_image(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid, const ls2fm_grid_desc* rad_grid,
                       const ls2fm_params* params, const float* poses, int32_t n_views, const float* kinv_host, int32_t height,
                       int32_t width, float* rgb, float* depth, float* normal, float* opacity, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sphere-traced depth and normal maps of whole images (new; the library's version stays ABI 13: the calls are additions).
 * Replaces: Camera.get_depth (pipelines/Camera.py:216-253): get_center_and_ray for every pixel, SDF.sphere_tracing
 * (models/SDF.py:149-214) over all of them and SDF.gradient (SDF.py:102-114) at the surface points -- without the track
 * ([R, iters_max+1, 3]), its re-evaluation or a second gradient query.
 * The rays are those ls2fm_camera_rays forms for poses and pix = 0 .. H*W-1 with width W (centres x + 0.5, y + 0.5).  Each view
 * gets the trip count K of the reference's loop over that view alone -- the trip at which its last start end finished -- and every
 * ray of the view sums the field over its first max(K, 1) track points, in ascending order.  Per view, every output is bit for bit
 * what ls2fm_sphere_trace + ls2fm_trace_depth_fwd (SDF.sphere_tracing(static_trips=True)) and ls2fm_sdf_eval's normal return:
 *   depth [n_views,H*W] = near + sum, clamped to far;  sdf_last [n_views,H*W]: the last value summed;
 *   finish uint8 [n_views,H*W] = |sdf_last| < finish_threshold;  points [n_views,H*W,3] = center + depth * ray (two roundings);
 *   gradient [n_views,H*W,3] or NULL: the analytic d sdf / d p at points;  t_end_k [n_views,H*W] or NULL: the far end after K
 *   trips;  trips int32 [n_views]: K of each view.  Row-major pixels.
 * poses [n_views,3,4] world-to-camera (DEVICE: read at run time); kinv_host: the 3 x 3 K^-1 as 9 HOST floats.
 * workspace: ls2fm_trace_image_workspace_bytes(...) bytes (the packed weights and one chunk of the normal query's sdf column):
 * it depends on nothing but the build, never on the image size or the number of views.  No allocation, no host
 * synchronisation, no stream fork: capturable.
 * Refusals (before any device work): LS2FM_ERR_UNSUPPORTED for bg_sdf; LS2FM_ERR_INVALID_ARGUMENT for null required pointers,
 * non-positive sizes or views, iters_max < 0 or 2^30 rays or more; LS2FM_ERR_WORKSPACE for a null workspace.  No gradients.
 */
int64_t ls2fm_trace_image_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid);
int ls2fm_trace_image(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                      const float* poses, int32_t n_views, const float* kinv_host, int32_t height, int32_t width,
                      float sdf_threshold, int32_t iters_max, float finish_threshold,
                      float* depth, float* sdf_last, uint8_t* finish, float* points, float* gradient,
                      float* t_end_k, int32_t* trips, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bidirectional sphere tracing, the no-grad root-find loop.
 * Replaces: the `while True` of SDF.sphere_tracing (models/SDF.py:149-200) including the AABB
 * near/far (SDF.py:120-122).  Each ray is advanced independently for up to iters_max trips and
 * records, per trip k, its pre-update start point (the reference's pts_track) and its far-end
 * distance; `trips` receives the GLOBAL trip count K of the reference's loop (min(iters_max, the
 * trip at which no start ray is unfinished)), which the caller uses to truncate the track.
 * Outputs: near, far [n_rays]; track [n_rays, iters_max+1, 3]; t_end [n_rays, iters_max+1];
 * trips int32[1]; track_sdf [n_rays, iters_max+1] or NULL: the field's value at every track point
 * -- what the re-evaluation of the track (SDF.py:203) returns, bit for bit (the loop has it for the
 * points it evaluated; a finished start end that still moves with its stale step is evaluated for
 * this output only).  The differentiable use of the track (SDF.py:203-214) is the caller's, through
 * the autograd-capable ops above.
 */
int ls2fm_sphere_trace(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                       const float* ray0, const float* ray_dir, int64_t n_rays, float sdf_threshold,
                       int32_t iters_max, float* near, float* far, float* track, float* t_end, float* track_sdf,
                       int32_t* trips, void* workspace, void* stream);

/* The two halves of ls2fm_sphere_trace for a caller that overlaps the tracing with other work: ls2fm_sdf_prepare packs the SDF
 * MLP's weights into `workspace` (weight-norm -> effective weights; one latency-bound workgroup, ~15 us) and zeroes *zero_word
 * (the tracing's `trips`; may be NULL); ls2fm_sphere_trace_prepared is ls2fm_sphere_trace without those two steps -- on any
 * stream ordered behind the prepare.  ls2fm.stage prepares on the step's stream and traces on another one beside the render's
 * gather pass (a one-workgroup prepare launched BESIDE that pass is starved: 15 -> 90 us, measured). */
int ls2fm_sdf_prepare(const ls2fm_grid_desc* grid, const ls2fm_params* params, void* workspace, int32_t* zero_word, void* stream);
int ls2fm_sphere_trace_prepared(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                                const float* ray0, const float* ray_dir, int64_t n_rays, float sdf_threshold,
                                int32_t iters_max, float* near, float* far, float* track, float* t_end, float* track_sdf,
                                int32_t* trips, void* workspace, void* stream);

/* ls2fm_sdf_eval (sdf only) with the packed weights a preceding ls2fm_sdf_eval / ls2fm_sphere_trace call left in `workspace`
 * (same stream, same parameters): no weight preparation launch.  Used between a tracing call and the evaluation of its track. */
int ls2fm_sdf_eval_prepared(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                            const float* p, int64_t n, float* sdf, const void* workspace, void* stream);

/* The tail of SDF.sphere_tracing for a ray batch (models/SDF.py:203-214) and the mask lines of CameraSet.render
 * (pipelines/Camera.py:515-516), with the trip count K read from the device (what ls2fm_sphere_trace left in `trips`): a
 * captured stage step never returns to the host.  sdf_tracks [n_rays][k_max] = the graph-enabled SDF values of the track points
 * (ls2fm_sdf_eval on `track`), k_max = iters_max.
 *   d_pred [n_rays]   = near + sum_{k < max(K,1)} sdf_tracks[r][k], replaced by far where it exceeds it
 *   sdf_last [n_rays] = sdf_tracks[r][max(K,1) - 1];   finish [n_rays] (u8) = |sdf_last| < finish_threshold
 *   rgb_gt [n_rays][3] (optional): mask_bg (u8) = bg_lo < mean(rgb_gt[r]) < bg_hi;  mask_dc (u8) = finish & mask_bg
 *   gate [n_rays] (u8): 1 where d_pred was not clamped (the backward's pass-through mask)
 * _bwd: d_sdf_tracks [n_rays][k_max] = (k < max(K,1) && gate[r]) * d_dpred[r] + (k == max(K,1) - 1) * d_sdf_last[r]; either
 * upstream may be NULL. */
int ls2fm_trace_depth_fwd(const float* sdf_tracks, const int32_t* trips, const float* near, const float* far, int64_t n_rays,
                          int32_t k_max, float finish_threshold, const float* rgb_gt, float bg_lo, float bg_hi, float* d_pred,
                          float* sdf_last, uint8_t* finish, uint8_t* mask_bg, uint8_t* mask_dc, uint8_t* gate, void* stream);
int ls2fm_trace_depth_bwd(const float* d_dpred, const float* d_sdf_last, const int32_t* trips, const uint8_t* gate,
                          int64_t n_rays, int32_t k_max, float* d_sdf_tracks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The re-projection term of a bundle-adjustment iteration and its gradient.
 * Replaces: the per-observation block of BA.run_ba (pipelines/BA.py:126-147) -- world2cam / cam2img of the surface-projected
 * tracked points through the live poses, the pixel error against their key points, the on-surface / finite mask, and the
 * robust mean of BA.compute_loss (BA.py:199-202) -- ~100 launch-bound PyTorch kernels per iteration with their autograd.
 *   points [n,3] (world); poses [n_views,3,4] world-to-camera (DEVICE); observations sorted by view: view v owns
 *   [view_start[v], view_start[v+1]) (DEVICE int32 [n_views+1]); intrinsic: HOST float[9], row-major K; obs_uv [n,2];
 *   sdf [n] or NULL: an observation counts when |sdf| < sdf_bound and its projection is not infinite.
 *   fwd -> err [n] (0 where not counted), on uint8 [n], sums DEVICE double[4] = {sum robust, sum err, count, reproj} with
 *   robust = 2 log(1 + err^2 / 4), reproj = 0.5 mean(robust) + 0.5 mean(err) over the counted ones (0 if none).
 *   bwd: d_reproj DEVICE float[1] -> d_points [n,3], d_poses [n_views,3,4] (overwritten; fixed-order sums, no atomics).
 *   workspace: ls2fm_reproject_workspace_bytes(n_views).
 */
int64_t ls2fm_reproject_workspace_bytes(int32_t n_views);
int ls2fm_reproject_fwd(const float* points, const float* poses, const int32_t* view_start, int32_t n_views,
                        const float* intrinsic, const float* obs_uv, const float* sdf, float sdf_bound, int64_t n,
                        float* err, uint8_t* on, double* sums, void* workspace, void* stream);
int ls2fm_reproject_bwd(const float* points, const float* poses, const int32_t* view_start, int32_t n_views,
                        const float* intrinsic, const float* obs_uv, const float* sdf, float sdf_bound, int64_t n,
                        const double* sums, const float* d_reproj, float* d_points, float* d_poses, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss head over the renderer's outputs: the scalar terms the reference's stages form
 * right after Renderer.forward, in one kernel each way instead of ~35 launch-bound PyTorch kernels.
 * Replaces: rgb L1 `l1_loss(rgb, rgbs_gt)` (pipelines/Camera.py:535); eikonal `l1_loss(norm(normals[mask]), 1)`
 * (Initialization.py:257-258, BA.py:193-194); depth consistency `smooth_l1_loss(d_points[mask_finish],
 * depth_mlp[mask_finish])`, 0 when the mask is empty (Camera.py:520-532); masked MSE behind PSNR (Camera.py:533);
 * the 10^w weighted sum of summarize_loss (BA.py:206-218).
 *   rgb, rgb_gt [n_rays,3]; normals [n_rays,n_samples,3]; depth [n_rays] (depth_mlp); depth_ref [n_rays] or NULL
 *   (sphere-traced d_points; NULL = no DC term); mask_* uint8 [n_rays] or NULL (= every ray): mask_eik selects the rays
 *   whose samples enter the eikonal mean, mask_dc = mask_finish, mask_mse = mask_bg.
 *   weights float[3] (DEVICE) = 10^w of (rgb, eikonal, DC).
 *   terms float[8] (DEVICE, overwritten) = {rgb L1 mean, eikonal mean, DC mean, masked MSE, weighted total, total again,
 *   PSNR = -10 log10(masked MSE) (Camera.py:534), 0}.
 *   sums double[8] (DEVICE, overwritten) = {S|rgb-gt|, n, S| |n|-1 |, n, S smooth_l1, n, S (rgb-gt)^2, n}: kept by the
 *   caller for the backward, and what a sharded run all-reduces for global normalisation.  Deterministic (fixed-order
 *   fp64 partials).  The workspace (ls2fm_loss_head_workspace_bytes) is zero-filled ONCE by the caller and reusable.
 * ls2fm_loss_head_bwd: d_terms float[5] = upstream gradient of `terms`, d_total float[1] = an additional upstream gradient
 * of the weighted total alone (either may be NULL = zeros, not both); writes (overwrites) d_rgb [n_rays,3],
 * d_normals [n_rays,n_samples,3], d_depth [n_rays] and, if non-NULL, d_depth_ref [n_rays].  Needs the `sums` of the
 * matching forward.
 */
int64_t ls2fm_loss_head_workspace_bytes(void);
int ls2fm_loss_head_fwd(const float* rgb, const float* rgb_gt, const float* normals, const float* depth,
                        const float* depth_ref, const uint8_t* mask_eik, const uint8_t* mask_dc, const uint8_t* mask_mse,
                        int64_t n_rays, int32_t n_samples, const float* weights, float* terms, double* sums, void* workspace,
                        void* stream);
int ls2fm_loss_head_bwd(const float* rgb, const float* rgb_gt, const float* normals, const float* depth,
                        const float* depth_ref, const uint8_t* mask_eik, const uint8_t* mask_dc, const uint8_t* mask_mse,
                        int64_t n_rays, int32_t n_samples, const float* weights, const float* d_terms, const float* d_total,
                        float* d_rgb, float* d_normals, float* d_depth, float* d_depth_ref, const double* sums, void* stream);
/* terms float[8] (DEVICE, overwritten) from sums double[8] (DEVICE) -- e.g. after a sharded run all-reduced the sums. */
int ls2fm_loss_terms_from_sums(const double* sums, const float* weights, float* terms, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Adam step over a list of fp32 tensors, one launch, one pass over memory.
 * Replaces: torch.optim.Adam.step() of the stage loops (Initialization.py:149-179, BA.py:117-182; amsgrad = False,
 * maximize = False):  g' = g + wd p;  m = lerp(m, g', 1 - beta1);  v = v beta2 + ((1 - beta2) g') g';
 * p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  lr, beta1 and beta2 are doubles (ABI 11), like torch's
 * hyper-parameters: 1 - beta, beta^step, lr / bc1 and sqrt(bc2) are formed in double and each is rounded to fp32 once.
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers; numel: HOST array; step >= 1 is the
 * count AFTER this update (torch increments before use).  Updates params, exp_avg, exp_avg_sq in place.
 */
int ls2fm_adam_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2, float eps,
                    float weight_decay, int64_t step, void* stream);

/* The same update with the schedule RESIDENT ON THE DEVICE, for optimisation steps captured into a hipGraph (a replay cannot
 * take a new learning rate or step count from the host).  sched_state: DEVICE, 32 bytes {double step, lr, gamma; float
 * step_size, bc2_sqrt} -- the caller initialises step = 0 (updates done so far), lr = the rate of the NEXT update and gamma =
 * ExponentialLR's factor (utils of the stage loops: BA.py:87-88, gamma = (lr_end / lr)^(1 / max_iter)); every call first
 * advances it (step += 1, bias corrections from the new step, lr *= gamma afterwards: optimizer.step() then scheduler.step())
 * in a one-thread kernel, then runs the update with those values.  Replaces torch.optim.Adam.step() + ExponentialLR.step().
 */
int ls2fm_adam_step_scheduled(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int64_t* numel, void* sched_state, double beta1, double beta2,
                              float eps, float weight_decay, void* stream);

/* Either update above with a MIRROR list: mirrors[t] (HOST array of n_tensors device pointers, entries may be NULL; NULL array =
 * none) is a second destination of tensor t's updated values in the entry-interleaved layout of ls2fm_interleave_tables /
 * ls2fm_params.dual_table -- element k goes to mirrors[t][(k >> 1) * 4 + (k & 1)], i.e. pass dual_table for the SDF table and
 * dual_table + 2 for the second field's table (8-byte aligned, even numel).  The render's gather pass reads that copy (one
 * 16-byte gather per corner serves both grids); writing it here, in the optimizer's one pass over the tables, keeps it current
 * without a rebuild per step.  sched_state NULL: the unscheduled form (lr and step from the arguments); otherwise the scheduled
 * form (lr and step ignored).  No reference counterpart: the reference's tcnn grids are separate.
 */
int ls2fm_adam_step_mirrored(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const int64_t* numel, float* const* mirrors, void* sched_state, double lr,
                             double beta1, double beta2, float eps, float weight_decay, int64_t step, void* stream);

/* The general form (the three above are special cases of it): every parameter GROUP of an optimizer in one call.  Per tensor t a
 * learning rate lrs[t] (HOST double array; with `step`, the unscheduled form) or a device-resident schedule sched_states[t] (HOST
 * array of DEVICE pointers, entries or the whole array may be NULL; every distinct schedule is advanced once per call);
 * mirrors as above or NULL.  Two tensors whose mirrors are the two halves of one interleaved copy (M and M + 2, equal length,
 * 16-byte aligned) -- the SDF table and the second field's table -- are updated by ONE job that also writes the copy as whole
 * 16-byte entries (full cache lines; two separate jobs would each write 8 bytes of every 16).  Replaces torch.optim.Adam.step()
 * over `[{sdf_func.parameters(), lr_sdf}, {color_func.parameters(), lr_color}]` (BA.py:79-83) + ExponentialLR.step().
 */
int ls2fm_adam_step_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, float* const* mirrors, const double* lrs,
                          void* const* sched_states, double beta1, double beta2, float eps, float weight_decay, int64_t step,
                          void* stream);

/* ExponentialLR.step() for parameter groups that took NO Adam step this iteration (every tensor's grad is None): the device
 * schedules' learning rates decay, `lr *= gamma`, their Adam step counts do not move -- torch's scheduler decays every group at
 * every step whether or not its tensors had gradients.  sched_states: HOST array of n DEVICE pointers (32-byte states as above).
 */
int ls2fm_adam_sched_decay(int32_t n, void* const* sched_states, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera rays: the pixels' camera centers and (unnormalised) ray directions through n_views pinhole cameras, one launch --
 * Camera.get_pts3D's ray construction and CameraSet.render's ray pick (pipelines/Camera.py:129-133, 457-463 on
 * utils/camera.py:230-252: get_center_and_ray = img2cam + cam2world) with, optionally, the se(3) -> SE(3) exponential map of
 * the live pose parameters in front (utils/camera.py:63-147: 11-term Taylor series, as BA.py:150-151 evaluates it every
 * iteration).  No gradients (the reference detaches the render poses, BA.py:150-151); same operation order as the torch code.
 *   poses [n_views,3,4] world-to-camera (device)  XOR  se3 [n_views,6] (w, u) (device);   kinv_host: the 3 x 3 K^-1 as 9 HOST floats
 *   pixels: xy [n,2] (or [n_views,n,2] with xy_per_view) device float coordinates  XOR  pix [n] int64 pixel indices of a
 *   width-`width` image (centres x + 0.5, y + 0.5: the same pixels in every view)
 *   view_sel: NULL, or a DEVICE int64[1]: only that view is processed (outputs have ONE view) -- a captured step follows the value
 *   centers, rays [n_views or 1, n, 3] (overwritten); poses_out [n_views or 1,3,4] or NULL: the poses used (se3 given: the exponentials)
 */
/* The exponential map alone, with its gradient: poses [n,3,4] = exp(se3 [n,6]) and d_se3 [n,6] from d_poses [n,3,4] (the chain
 * rule through the truncated series, term by term, as autograd differentiates utils/camera.py:63-147) -- the live poses of a
 * bundle-adjustment iteration that the re-projection term reads (BA.py:126-147), one launch each way instead of ~90. */
int ls2fm_se3_exp_fwd(const float* se3, int32_t n, float* poses, void* stream);
int ls2fm_se3_exp_bwd(const float* se3, const float* d_poses, int32_t n, float* d_se3, void* stream);
int ls2fm_camera_rays(const float* poses, const float* se3, const float* kinv_host, const float* xy, const int64_t* pix,
                      int32_t width, int32_t xy_per_view, const int64_t* view_sel, int32_t n_views, int64_t n, float* centers,
                      float* rays, float* poses_out, void* stream);

/* The tracing-consistency term of a stage-loop iteration -- the traced key points' surface points against their tracked 3-D
 * points (pipelines/Camera.py:108-143 get_pts3D and the callers' loss lines, e.g. BA.py:155-161) -- as one launch each way:
 *   surface_i = center_i + ray_i d_i ;  w_i = live_i / sum(live) ;  out[0] = sum_i |target_i - surface_i| w_i ;
 *   out[1] = sum_i |sdf_last_i| w_i (0 when sdf_last is NULL) ;  out[2] = sum(live)            (fp64 fixed-order sums)
 * center, ray, target [n,3], d, live, sdf_last [n] (device); out [3].  bwd: g_tl, g_sd: one float each, the upstreams of out[0]
 * and out[1] (device; NULL = that term has no upstream: zero) -> d_d [n], d_sdf [n] (NULL with sdf_last NULL); d |e| / d d at
 * e = 0 is 0, sign(0) = 0, as torch.  No live row: out[0], out[1] are 0 / 0 = NaN and so is EVERY gradient entry, as torch's. */
int ls2fm_tracing_term_fwd(const float* center, const float* ray, const float* d, const float* target, const float* live,
                           const float* sdf_last, int64_t n, float* out, void* stream);
int ls2fm_tracing_term_bwd(const float* center, const float* ray, const float* d, const float* target, const float* live,
                           const float* sdf_last, int64_t n, const float* out, const float* g_tl, const float* g_sd, float* d_d,
                           float* d_sdf, void* stream);

/* The loss lines of a bundle-adjustment iteration outside the render (pipelines/BA.py:160-170: `sdf_surf`, the adaptive weight
 * 10^1 of the re-projection error above 10 px, the weighted sum) as one launch each way:
 *   out_surf = mean |sdfs| ;  out_w = reproj > thresh ? w_hi : w_lo  (from the error's VALUE: no gradient through the choice) ;
 *   out_extra = out_w reproj + w_surf out_surf + w_add add        (add: one more device scalar, e.g. the tracing loss; may be NULL)
 * reproj, add, the three outputs: one float each (device); sdfs [n].  bwd: g [1] upstream of out_extra ->
 * d_reproj [1] = g out_w, d_sdfs [n] = g w_surf sign(sdfs) / n (sign(0) = 0, as torch), d_add [1] = g w_add (NULL with add NULL). */
int ls2fm_ba_terms_fwd(const float* reproj, const float* sdfs, int64_t n, const float* add, float thresh, float w_lo, float w_hi,
                       float w_surf, float w_add, float* out_surf, float* out_w, float* out_extra, void* stream);
int ls2fm_ba_terms_bwd(const float* sdfs, int64_t n, const float* w_reproj, const float* g, float w_surf, float w_add,
                       float* d_reproj, float* d_sdfs, float* d_add, void* stream);

/* out[0] = wa a[0] + wb b[0] of two device scalars (the loops' weighted sums of two loss terms, e.g. Initialization.py:252-255);
 * bwd: d2[0] = g[0] wa, d2[1] = g[0] wb (one two-float buffer).  One launch each way instead of five elementwise kernels. */
int ls2fm_weighted_pair_fwd(const float* a, const float* b, float wa, float wb, float* out, void* stream);
int ls2fm_weighted_pair_bwd(const float* g, float wa, float wb, float* d2, void* stream);

/* SDF.get_surface_pts' projection line (models/SDF.py:104-110):  out = p - normals / |normals|.detach() * sdf ,  length = |normals|
 * (p, normals, out [n,3]; sdf, length [n]) and its gradient w.r.t. normals and sdf (d p = g_out, the caller's); g_out / g_length
 * may be NULL (no upstream for that output).  One launch each way instead of ~14 elementwise kernels. */
int ls2fm_surface_pts_fwd(const float* p, const float* normals, const float* sdf, int64_t n, float* out, float* length, void* stream);
int ls2fm_surface_pts_bwd(const float* normals, const float* sdf, const float* length, int64_t n, const float* g_out,
                          const float* g_length, float* d_normals, float* d_sdf, void* stream);

/* The explicit-match terms of the two-view initialisation (pipelines/Initialization.py:154-160, 252-255; Camera.py:136, 168-178):
 * n_seg <= 4 segments of n traced key points each (segment = source view); pts = center + ray d is projected through
 * poses[seg] (the OTHER view's world-to-camera [3,4], device, no gradient) and K and compared with uv_obs:
 *   out[0] = mean || uv(pts) - uv_obs ||   out[1] = mean |sdf_last|   over all n_seg * n points;  surface [n_seg * n, 3] = pts.
 * center, ray [n_seg * n, 3], uv_obs [n_seg * n, 2] (device); d, sdf_last, d_d, d_sdf: HOST arrays of n_seg DEVICE pointers ([n] each);
 * g [2] (device): upstream of out[0], out[1].  One launch each way instead of ~70 torch kernels. */
int ls2fm_match_term_fwd(const float* center, const float* ray, const float* uv_obs, const float* poses, const float* intrinsic_host,
                         int32_t n_seg, int64_t n, const float* const* d, const float* const* sdf_last, float* surface, float* out,
                         void* stream);
int ls2fm_match_term_bwd(const float* center, const float* ray, const float* uv_obs, const float* poses, const float* intrinsic_host,
                         int32_t n_seg, int64_t n, const float* const* d, const float* const* sdf_last, const float* g,
                         float* const* d_d, float* const* d_sdf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Absolute pose (csrc/absolute_pose.hip): what Registration.PnP asks of pycolmap (pipelines/Registration.py:94-109,
 * absolute_pose_estimation + pose_refinement), for many views in one call.  All geometry in fp64.  Poses are world-to-camera
 * [3,4] = [R | t] row-major; a pinhole view v has intr[v] = (fx, fy, cx, cy) (DEVICE doubles); pixel of a camera point p:
 * (fx p.x / p.z + cx, fy p.y / p.z + cy).  Correspondences are sorted by view: view v owns [view_start[v], view_start[v + 1])
 * (DEVICE int32 [n_views + 1], non-decreasing; the ragged convention of ls2fm_reproject_*).  tests/pose_restate.py repeats every
 * rule below in numpy.
 *
 * ls2fm_p3p: m minimal problems, each 3 unit bearings [m][3][3] and 3 world points [m][3][3] (device) -> up to 4 poses
 * [m][4][3][4] (the kept ones first, in slot order; the rest zero) and n_solutions [m].  Lambda Twist (Persson & Nordberg, ECCV
 * 2018): the cubic det(D1 + g D2) = 0 of the two homogeneous distance forms (its only real root, or the largest of three; two
 * Newton steps), the degenerate conic's two lines (slots 0-1: w = e1 - r e2, slots 2-3: w = e1 + r e2), each met with the other
 * form (roots q / C, then A / q), depths scaled on the longest side and polished by <= 5 Gauss-Newton steps on the three distance
 * equations; R from the two triangles' orthonormal frames, t from the centroids.  A solution with a sample point at camera
 * z <= 0 or a non-finite entry is dropped; collinear or coincident points (|d01 x d02|^2 <= 1e-20 |d01|^2 |d02|^2) give 0
 * solutions, never NaN.
 *
 * ls2fm_absolute_pose: LO-RANSAC per view (samples, scoring, selection and rounds are csrc/ransac.h's, which the relative pose
 * shares).
 *   samples   trial t (0, 1, 2, ... per view) draws indices from key = splitmix64(seed ^ splitmix64(t)): draw k is
 *             ((splitmix64(key + k) >> 32) * n) >> 32 over the view's n correspondences; the sample is the first three distinct
 *             values among draws k = 0 .. 63 (none: the trial has no pose).  splitmix64(x): z = x + 0x9E3779B97F4A7C15;
 *             z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)  (mod 2^64).
 *             The view's position in the batch is not part of the key: a view draws the same samples alone or in any batch.
 *   hypotheses ls2fm_p3p of the sample's bearings normalise((u - cx) / fx, (v - cy) / fy, 1); slot s = the P3P slot above.
 *   scoring   correspondence i is an inlier of P when its camera z > 0 and its squared pixel error < max_error_px^2; counts are
 *             exact integers.
 *   selection the best (count, then lowest t * 4 + s) over all trials so far: the 64-bit max of (count << 32 | ~(t * 4 + s)).
 *   rounds    trials run in rounds of LS2FM_POSE_ROUND per view still active; after a round, with eps = best count / n,
 *             N = clamp(ceil(log(1 - confidence) / log(1 - eps^3)), min(min_num_trials, cap), cap) (eps = 0: cap; eps = 1: the
 *             lower bound), cap = min(max_num_trials, the same formula at eps = min_inlier_ratio): the cap wins over min_num_trials,
 *             as in COLMAP's RANSAC.  The view stops once its trials >= N.  The
 *             host reads one "views still active" word per round: the call SYNCHRONISES and is not capturable.
 *   local optimisation from the best pose, up to 10 times: Gauss-Newton step on the inliers' squared pixel error (increment
 *             (w, dt): R <- exp([w]x) R, t <- exp([w]x) t + dt; 6 x 6 normal equations reduced in a fixed order, Cholesky),
 *             recount; the step is kept when its count is >= the old one, and the loop stops when it is not, when fewer than 3
 *             inliers remain or when the inlier set did not change.  inliers[] (uint8) = the final set.
 *   refinement (opts->refine) ls2fm_pose_refine's loop on that fixed set, loss scale 1 px, LS2FM_POSE_REFINE_ITERS iterations.
 *   outputs   poses [V][3][4], num_inliers, trials (run), best_trial (the winning SAMPLED trial t, before local optimisation;
 *             -1 when none), success = num_inliers >= 4.  A view with n < 3 (or no hypothesis with an inlier) fails: identity
 *             pose, 0 inliers, without touching its neighbours.  Every bit depends on the view's own data, seed and options only.
 *   options   max_error_px > 0, 0 < confidence < 1, 0 <= min_inlier_ratio < 1, 0 <= min_num_trials <= max_num_trials,
 *             1 <= max_num_trials <= LS2FM_POSE_MAX_TRIALS, refine 0 / 1; 1 <= n_views <= LS2FM_POSE_MAX_VIEWS.  A refusal
 *             returns LS2FM_ERR_INVALID_ARGUMENT and launches nothing.  workspace: ls2fm_absolute_pose_workspace_bytes
 *             (~400 KB per view; n_corr does not change it).
 *
 * ls2fm_pose_refine: pose_refinement on a FIXED mask (uint8 per correspondence): Levenberg-Marquardt on 0.5 sum rho(s_i),
 * s_i = squared pixel error, Cauchy rho(s) = c^2 log(1 + s / c^2) with c = loss_scale_px, normal equations weighted by rho'(s);
 * damping lambda diag(H) (diagonal floored at 1e-12 of its largest entry), lambda = 1e-4 at the start, x 0.1 after a step that
 * lowers the cost, x 10 after one that does not; at most max_iters iterations; stops when max |gradient| <= 1e-10 or after a kept
 * step with max |increment| <= 1e-12 (1 + max |t|).  Views with fewer than 3 masked correspondences keep their pose.  One
 * workgroup per view, fixed-order sums: repeatable bit for bit, and capturable (it reads nothing back).
 */
#define LS2FM_POSE_ROUND 1024
#define LS2FM_POSE_MAX_VIEWS 65535
#define LS2FM_POSE_MAX_TRIALS (1 << 24)
#define LS2FM_POSE_REFINE_ITERS 100

typedef struct ls2fm_pose_ransac_opts {
    double max_error_px;
    double confidence;
    double min_inlier_ratio;
    int64_t min_num_trials;
    int64_t max_num_trials;
    uint64_t seed;
    int32_t refine;
} ls2fm_pose_ransac_opts;

int ls2fm_p3p(const double* bearings, const double* points, int64_t m, double* poses, int32_t* n_solutions, void* stream);
int64_t ls2fm_absolute_pose_workspace_bytes(int32_t n_views, int64_t n_corr);
int ls2fm_absolute_pose(const double* uv, const double* xyz, const int32_t* view_start, int32_t n_views, const double* intr,
                        const ls2fm_pose_ransac_opts* opts, double* poses, uint8_t* inliers, int32_t* num_inliers, int32_t* trials,
                        int32_t* best_trial, int32_t* success, void* workspace, void* stream);
int ls2fm_pose_refine(const double* uv, const double* xyz, const int32_t* view_start, int32_t n_views, const double* intr,
                      const uint8_t* mask, const double* poses_in, float loss_scale_px, int32_t max_iters, double* poses_out,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Relative pose (csrc/relative_pose.hip): what Initializer asks of pycolmap (pipelines/Initialization.py:86-95,
 * essential_matrix_estimation) and the _Trad drivers of cv2 (triangulatePoints), for many view pairs in one call.  All geometry in
 * fp64.  Normalised image point of pixel (u, v) under (fx, fy, cx, cy): x = ((u - cx) / fx, (v - cy) / fy).  E (row-major 3 x 3)
 * maps camera 1 to camera 2: x2h^T E x1h = 0 for X2 = R X1 + t, E ~ [t]x R.  Correspondences are sorted by pair: pair p owns
 * [pair_start[p], pair_start[p + 1]) of uv0 / uv1 [n][2] (DEVICE int32 [n_pairs + 1], non-decreasing, the ragged convention of
 * ls2fm_absolute_pose's view_start); intr0 / intr1 [n_pairs][4] are each pair's two cameras.  tests/relpose_restate.py repeats
 * every rule below in numpy.
 *
 * ls2fm_five_point: m minimal problems, x1 / x2 [m][5][2] normalised points -> up to 10 essential matrices E [m][10][3][3] (the
 * kept ones first, zero beyond) and n_solutions [m].  Nister (CVPR 2003 / PAMI 2004) as COLMAP implements it:
 *   null space  Gauss-Jordan with partial pivoting on the 5 x 9 rows kron((x2, 1), (x1, 1)); a column whose largest remaining
 *               |entry| is <= 1e-12 of the matrix's largest is free; rank != 5 gives 0 solutions.  Basis vector j (free column
 *               f_j, ascending): 1 at f_j, -R[i][f_j] at pivot column i; modified Gram-Schmidt in order j = 0..3 -> X, Y, Z, W.
 *   constraints E = x X + y Y + z Z + W; det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20 matrix over the cubic monomials
 *               x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
 *   elimination Gauss-Jordan with partial pivoting of the left 10 x 10 block (pivot <= 1e-14 of the largest entry: 0 solutions)
 *               -> [I | AA]; B(z) [x y 1]^T = 0 from rows (x^2z, x^2), (y^2z, y^2), (xyz, xy) as <e> - z <f> (degrees 3, 3, 4).
 *   roots       det B(z), degree 10 (ascending coefficients, each Sturm polynomial divided by its largest |coefficient|): the
 *               Sturm sequence p0, p0', -rem(...) (a remainder's trailing coefficients with |c| <= LS2FM_STURM_TRIM are dropped),
 *               the Cauchy bound 1 + max |c_i / c_d|, the k-th real root by bisection on the sign-variation count (at most 100
 *               halvings, until the bracket is <= LS2FM_BISECT_TOL max(1, |lo|, |hi|)), then <= 5 Newton steps on p0 that stay
 *               inside the bracket.  No eigen solve.
 *   recovery    per root z (ascending): the unit null vector of B(z) (the largest cross product of two rows), skipped when
 *               |X_3| < 1e-10; E = x X + y Y + z Z + W with x = X_1 / X_3, y = X_2 / X_3, scaled to unit Frobenius norm with its
 *               largest |entry| (the first of equals, row-major) positive.  Non-finite solutions are dropped.
 *   Degenerate samples (coincident points, a rank-deficient system) give 0 solutions, never NaN.
 *
 * ls2fm_relative_pose: LO-RANSAC per pair (the rounds of csrc/ransac.h, as ls2fm_absolute_pose).
 *   samples   ls2fm_absolute_pose's SplitMix64 stream keyed by (seed, trial); the sample is the first FIVE distinct draws among
 *             k = 0 .. 63 (none: the trial has no model).
 *   hypotheses ls2fm_five_point of the sample; slot s = the solution's place (0..9).
 *   scoring   squared Sampson error in normalised coordinates, (x2h^T E x1h)^2 / ((E x1h)_1^2 + (E x1h)_2^2 + (E^T x2h)_1^2 +
 *             (E^T x2h)_2^2); an inlier when it is <= max_error^2, max_error = 0.5 (max_error_px / f1 + max_error_px / f2), f the
 *             camera's (fx + fy) / 2 (COLMAP).  Counts are exact integers.
 *   selection the 64-bit max of (count << 32 | ~(t * 10 + s)): the best count, then the lowest t * 10 + s.
 *   rounds    as ls2fm_absolute_pose with eps^5 for eps^3: N = clamp(ceil(log(1 - confidence) / log(1 - eps^5)), min(min_num_trials,
 *             cap), cap); the cap wins over min_num_trials.  The call SYNCHRONISES (one word per round) and is not capturable.
 *   local optimisation from the best E, up to 10 times while >= 5 inliers: the 9 x 9 normal matrix of the inliers' rows
 *             kron((x2, 1), (x1, 1)) (fixed-order sum), its eigenvectors by cyclic Jacobi (<= 30 sweeps), the four of the smallest
 *             eigenvalues (the lower index first among equals) as W, Z, Y, X, the five-point steps above from the constraints on;
 *             each candidate is recounted, the best (count, then lowest slot) is kept when its count is >= the current one, and
 *             the loop stops when it is lower, when there is no candidate, or when the inlier set did not change.
 *   pose      COLMAP's PoseFromEssentialMatrix: E = U diag V^T (one-sided Jacobi; U, V proper), R1 = U W V^T, R2 = U W^T V^T,
 *             t = U col 3, W = [0 1 0; -1 0 0; 0 0 1]; candidates (R1, t), (R2, t), (R1, -t), (R2, -t); each inlier is
 *             triangulated (ls2fm_triangulate's DLT with [I | 0] and [R | t]) and counted when its depth is in
 *             (DBL_EPSILON, 1000 |R^T t|) in both cameras; the candidate with the most points wins (ties: the later one).
 *   outputs   E [P][3][3], poses [P][3][4] = [R | t] (X2 = R X1 + t, |t| = 1), inliers (uint8) of the final E, num_inliers,
 *             trials, best_trial (the winning SAMPLED trial, -1 when none), success = num_inliers >= 5 and >= 1 point in front.
 *             A failing pair gets the identity pose (E zero when no hypothesis had an inlier), without touching its neighbours;
 *             every bit depends on the pair's own data, seed and options only.
 *   options   ls2fm_pose_ransac_opts with refine == 0 (no refinement is defined for E); otherwise as ls2fm_absolute_pose;
 *             1 <= n_pairs <= LS2FM_RELPOSE_MAX_PAIRS.  A refusal returns LS2FM_ERR_INVALID_ARGUMENT and launches nothing.
 *             workspace: ls2fm_relative_pose_workspace_bytes (~780 KB per pair; n_corr does not change it).
 *
 * ls2fm_triangulate: two-view DLT of n points, one thread each: P0 / P1 [n_pairs][3][4] (any projection matrices), pixel pairs
 * uv0 / uv1 [n][2] sorted by pair (pair_start as above) -> X [n][4] homogeneous.  A = the 4 x 4 of cv2.triangulatePoints (rows
 * u P[2] - P[0], v P[2] - P[1] of each view); the right singular vector of its smallest singular value by one-sided Jacobi on A
 * (<= 30 sweeps; rotations while |a_p . a_q| > 1e-15 |a_p| |a_q|), unit norm, w >= 0 (cv2's up to sign).  Capturable.
 */
#define LS2FM_FIVE_POINT_MAX_SOLUTIONS 10
#define LS2FM_RELPOSE_MAX_PAIRS 65535
#define LS2FM_STURM_TRIM 1e-14
#define LS2FM_BISECT_TOL 1e-10

int ls2fm_five_point(const double* x1, const double* x2, int64_t m, double* E, int32_t* n_solutions, void* stream);
int64_t ls2fm_relative_pose_workspace_bytes(int32_t n_pairs, int64_t n_corr);
int ls2fm_relative_pose(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs, const double* intr0,
                        const double* intr1, const ls2fm_pose_ransac_opts* opts, double* E, double* poses, uint8_t* inliers,
                        int32_t* num_inliers, int32_t* trials, int32_t* best_trial, int32_t* success, void* workspace, void* stream);
int ls2fm_triangulate(const double* P0, const double* P1, const double* uv0, const double* uv1, const int32_t* pair_start,
                      int32_t n_pairs, int64_t n, double* X, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Uncalibrated two-view geometry (csrc/two_view.hip; additions, the library stays ABI 13): the fundamental matrix and the
 * homography of COLMAP's two-view geometry for many view pairs in one call, in PIXELS -- no intrinsics.  All geometry in fp64.
 * F (row-major 3 x 3) has x2h^T F x1h = 0 and H has x2h ~ H x1h for pixels x1 of the first and x2 of the second image.  The ragged
 * pair_start convention, the options struct and the rounds are ls2fm_relative_pose's.  tests/twoview_restate.py repeats every rule
 * below in numpy.
 *
 * conditioning (both minimal solvers and both local optimisations, per image): Hartley normalisation of the point set at hand:
 *   c = (sum x) / n ; d2 = sum |x - c|^2 ; s = sqrt(2) / sqrt(d2 / n) ; x_n = s (x - c), i.e. T = [s 0 -s cx; 0 s -s cy; 0 0 1].
 *   A set whose sqrt(d2 / n) is 0 or not finite yields no model.  A model M_n between normalised points is de-normalised
 *   (F = T2^T F_n T1, H = T2^-1 H_n T1), scaled to unit Frobenius norm and signed so that its largest |entry| (the first of equals,
 *   row-major) is positive; a model that is zero or not finite after that is dropped.
 *
 * ls2fm_seven_point: m minimal problems, uv0 / uv1 [m][7][2] pixels -> F [m][3][3][3] (kept ones first, zero beyond) and
 * n_solutions [m].
 *   null space  the 7 x 9 rows kron((x2_n, 1), (x1_n, 1)) by ls2fm_five_point's Gauss-Jordan rule (partial pivoting; a column whose
 *               largest remaining |entry| is <= 1e-12 of the matrix's largest is free; basis vector j for free column f_j,
 *               ascending: 1 at f_j, -R[i][f_j] at pivot column i; modified Gram-Schmidt in order j = 0, 1) -> F1, F2.  rank != 7: 0
 *               solutions.
 *   cubic       det(l F1 + (1 - l) F2) = det(F2 + l (F1 - F2)), expanded multilinearly in the rows; its coefficients divided by
 *               the largest |coefficient|; |c3| < 1e-14 then: a quadratic (|c2| < 1e-14 as well: linear, c1 = 0: no root).
 *   roots       CLOSED FORM plus a bracketed Newton polish (not the Sturm machinery of ls2fm_five_point).  Monic a, b, d;
 *               Q = (a^2 - 3 b) / 9, R = (2 a^3 - 9 a b + 27 d) / 54, mid = -a / 3.  R^2 < Q^3: three roots
 *               mid - 2 sqrt(Q) cos((th + 2 pi k) / 3), th = acos(R / sqrt(Q^3)), k = 0, -1, 1, bracketed by the turning points
 *               (-inf, mid - sqrt Q], [mid - sqrt Q, mid + sqrt Q], [mid + sqrt Q, inf).  Otherwise one root
 *               mid + A + Q / A, A = -sign(R) cbrt(|R| + sqrt(R^2 - Q^3)), bracketed on its side of the turning points when
 *               Q > 0.  A quadratic: q = -(c1 + sign(c1) sqrt(disc)) / 2, roots q / c2 and c0 / q, bracketed by the vertex.  Each
 *               root takes <= 5 Newton steps on the scaled polynomial; a step that leaves its bracket, does not move or meets a
 *               zero derivative ends the polish.  Roots ascending.
 *   recovery    F_n = l F1 + (1 - l) F2 per root, the conditioning block's de-normalisation, norm and sign.
 *
 * ls2fm_four_point_homography: m problems uv0 / uv1 [m][4][2] -> H [m][3][3], n_solutions [m] (0 or 1).  DLT: per correspondence
 *   the rows (-x, -y, -1, 0, 0, 0, u x, u y, u) and (0, 0, 0, -x, -y, -1, v x, v y, v) of (x, y) = x1_n, (u, v) = x2_n; the null
 *   vector by the same Gauss-Jordan rule; rank != 8 (three collinear points, coincident points): 0 solutions.
 *
 * ls2fm_fundamental_matrix / ls2fm_homography: LO-RANSAC per pair (the rounds of csrc/ransac.h).
 *   samples   ls2fm_absolute_pose's SplitMix64 stream keyed by (seed, trial): the first 7 (F) / 4 (H) distinct draws among
 *             k = 0 .. 63.  hypotheses: the minimal solver of the sample, slot s = the solution's place (F: 0..2, H: 0).
 *   scoring   F: squared Sampson error in pixels (ls2fm_relative_pose's formula on pixel coordinates) <= max_error_px^2.
 *             H: |pi(H x1h) - x2|^2 <= max_error_px^2; a correspondence whose (H x1h)_3 has |.| <= DBL_EPSILON or is not finite is
 *             not an inlier.  Counts are exact integers.
 *   selection the 64-bit max of (count << 32 | ~(t * S + s)), S = 3 (F) / 1 (H).
 *   rounds    as ls2fm_relative_pose with eps^7 (F) / eps^4 (H).  The call SYNCHRONISES (one word per round), not capturable.
 *   local optimisation from the best model, up to 10 times while >= 8 (F) / >= 4 (H) inliers: the conditioning of the inlier set
 *             (fixed-order sums), the 9 x 9 normal matrix of the inliers' normalised rows (F: the row kron((x2_n, 1), (x1_n, 1));
 *             H: the two DLT rows; fixed-order sum), its eigenvector of the smallest eigenvalue by ls2fm_relative_pose's cyclic
 *             Jacobi (the lower index first among equals); for F the smallest singular value zeroed in normalised coordinates
 *             (one-sided Jacobi on the columns, the lower index among equal column norms); de-normalised, unit norm, signed; the
 *             candidate is recounted and kept when its count is >= the current one; the loop stops when it is lower, when there
 *             is no candidate, or when the inlier set did not change.
 *   outputs   model [P][3][3], inliers (uint8) of the final model, num_inliers, trials, best_trial (the winning SAMPLED trial, -1
 *             when none), success = num_inliers >= 8 (F) / >= 4 (H).  A pair without success gets a ZERO matrix, an all-zero mask
 *             and num_inliers 0 (trials and best_trial still tell what ran; a pair below the sample size has trials 0), without
 *             touching its neighbours; every bit depends on the pair's own data, seed and options only.
 *   options   ls2fm_pose_ransac_opts with refine == 0; limits and refusals as ls2fm_relative_pose.  workspace:
 *             ls2fm_fundamental_matrix_workspace_bytes (~230 KB per pair) / ls2fm_homography_workspace_bytes (~80 KB per pair).
 */
#define LS2FM_SEVEN_POINT_MAX_SOLUTIONS 3

int ls2fm_seven_point(const double* uv0, const double* uv1, int64_t m, double* F, int32_t* n_solutions, void* stream);
int ls2fm_four_point_homography(const double* uv0, const double* uv1, int64_t m, double* H, int32_t* n_solutions, void* stream);
int64_t ls2fm_fundamental_matrix_workspace_bytes(int32_t n_pairs, int64_t n_corr);
int64_t ls2fm_homography_workspace_bytes(int32_t n_pairs, int64_t n_corr);
int ls2fm_fundamental_matrix(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs,
                             const ls2fm_pose_ransac_opts* opts, double* F, uint8_t* inliers, int32_t* num_inliers, int32_t* trials,
                             int32_t* best_trial, int32_t* success, void* workspace, void* stream);
int ls2fm_homography(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs,
                     const ls2fm_pose_ransac_opts* opts, double* H, uint8_t* inliers, int32_t* num_inliers, int32_t* trials,
                     int32_t* best_trial, int32_t* success, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Classical bundle adjustment over explicit points and se(3) poses (new; the library's version stays ABI 13: the calls are additions): the loop of pipelines/BA_Trad.py:86-130
 * (`BA.run_ba` behind Ablate_config.ba_trad) -- n_iters iterations in ONE call, two plain launches each, no host read inside.
 *   iteration pose_v = se3_to_SE3(se3[v]) (ls2fm_se3_exp_fwd's arithmetic) ; x_c = R x + t ; u = K x_c ; uv = u_xy / (u_z + 1e-6) ;
 *             err = |uv - obs_uv| ; reproj = 0.5 mean(2 log(1 + err^2 / 4)) + 0.5 mean(err) over ALL n_obs observations (fp32 per
 *             observation in ls2fm_reproject_fwd's order, fp64 fixed-order sums) ; w = reproj > thresh ? w_hi : w_lo ; the
 *             gradient of w reproj w.r.t. se3 (ls2fm_se3_exp_bwd's arithmetic) and the points (a point's observations summed in
 *             list order: no floating-point atomics, a run repeats itself bit for bit) ; torch.optim.Adam's update (defaults:
 *             betas 0.9 / 0.999, eps 1e-8; the element arithmetic of ls2fm_adam_step) with the rates lr_rot (se3[:, 0:3]),
 *             lr_trans (se3[:, 3:6]) and lr_points, each multiplied by gamma after every iteration (ExponentialLR).  A point
 *             without an observation is not touched (value and moments).
 *   prepare   ls2fm_bundle_adjust_prepare, ONCE per loop (it synchronises `stream`; not capturable): view_start [V + 1] (int32,
 *             device; view v owns observations view_start[v] : view_start[v + 1]) and obs_point [n_obs] (int32, device; the point
 *             each observation sees) are read back, checked, and copied into `workspace` together with the point -> observations
 *             lists.  LS2FM_ERR_INVALID_ARGUMENT: n_obs < 1, n_views < 1, n_points < 1, view_start[0] != 0, view_start[V] != n_obs,
 *             a view without an observation, an obs_point outside [0, n_points).  The kernels index through the workspace's
 *             copies only.  workspace: ls2fm_bundle_adjust_workspace_bytes (negative for sizes that are refused).
 *   run       ls2fm_bundle_adjust_run: se3 [V][6] and points [P][3] are updated in place; m_* / v_* are Adam's moment buffers
 *             (zero before the first iteration) and steps_done the number of iterations already taken on them -- both owned by
 *             the caller, so 2 calls of 10 iterations equal 1 call of 20 bit for bit.  intrinsic_host: K as 9 HOST floats.
 *             log [n_iters][3] (device): reproj, w, mean(err) of every iteration.  se3_entering_last [V][6] / points_entering_last
 *             [P][3]: the state that ENTERED the call's last iteration (what BA_Trad writes back after its loop, BA_Trad.py:124-127;
 *             log[n_iters - 1][2] is the value it returns); se3 / points hold the state after the last Adam step.
 *             LS2FM_ERR_INVALID_ARGUMENT: n_iters < 1, null buffers, sizes as above; LS2FM_ERR_WORKSPACE: null workspace;
 *             LS2FM_ERR_UNSUPPORTED: `stream` is capturing (the per-iteration scalars come from the host's step count).  A
 *             workspace that prepare did not fill for these sizes moves nothing and logs NaN.
 */
int64_t ls2fm_bundle_adjust_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs);
int ls2fm_bundle_adjust_prepare(const int32_t* view_start, int32_t n_views, const int32_t* obs_point, int64_t n_obs, int64_t n_points,
                                void* workspace, void* stream);
int ls2fm_bundle_adjust_run(float* se3, float* points, const float* obs_uv, int32_t n_views, int64_t n_points, int64_t n_obs,
                            const float* intrinsic_host, double lr_rot, double lr_trans, double lr_points, double gamma, float w_lo,
                            float w_hi, float thresh, float* m_se3, float* v_se3, float* m_points, float* v_points, int64_t steps_done,
                            int32_t n_iters, float* log, float* se3_entering_last, float* points_entering_last, void* workspace,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * Levenberg-Marquardt bundle adjustment with a Schur complement (csrc/bundle_adjust_lm.hip; additions, the library stays ABI 13):
 * explicit points and [R | t] poses of V <= LS2FM_BA_LM_MAX_VIEWS picked views, one shared pinhole camera, all arithmetic fp64, no
 * floating-point atomics, every sum in a fixed order.  tests/ba_lm_restate.py repeats every rule in numpy, by two routes.
 *   model     x_c = R X + t ; r = (fx x/z + cx - u, fy y/z + cy - v), a plain division ; s = |r|^2 ; rho(s) with scale c:
 *             loss 0 (trivial) rho = s ; 1 (soft_l1) rho = 2 c^2 (sqrt(1 + s / c^2) - 1) ; 2 (cauchy) rho = c^2 log(1 + s / c^2).
 *             cost = 1/2 sum rho(s) over ALL observations.  IRLS weight w = rho'(s), no second-order correction.
 *   step      pose perturbation (omega, dt): d x_c = -[x_c]x omega + dt, the update R <- exp([omega]x) R, t <- exp([omega]x) t + dt
 *             (ls2fm_pose_refine's); J_c 2 x 6, J_p = J_proj R 2 x 3.  A constant view has J_c = 0; a point with fewer than
 *             min_point_views observations among the picked views has J_p = 0 (its observations still constrain their cameras and
 *             count in the cost).  U_v = sum w J_c^T J_c, g_v = sum w J_c^T r over the view's observations in list order; V_p, g_p
 *             over the point's observations in list order; W_o = w J_c^T J_p.  Damping per block: B* = B + lambda diag(max(B_kk,
 *             1e-12 max_k B_kk)).  Reduced system S_ij = [i = j] U_i* - sum_p W_ip V_p*^-1 W_jp^T, b_i = -(g_i - sum_p W_ip V_p*^-1
 *             g_p), a constant view's block the identity with right-hand side 0; S delta_c = b by Cholesky (dense, 6-column
 *             panels); delta_p = -V_p*^-1 (g_p + sum_o W_o^T delta_c[view(o)]), 0 for a constant point.
 *   decision  the candidate (updated poses, X + delta_p) is accepted iff its cost < the current cost (strict: a non-finite
 *             candidate is rejected): lambda <- max(0.1 lambda, 1e-16); otherwise, or after a non-positive Cholesky pivot (of S or
 *             of a V_p*), lambda <- 10 lambda.  The loop stops (reason) when max |g| <= grad_tol (1; checked first, the state
 *             stays), an accepted step has max |delta| <= step_tol (1 + max |parameter|) (2; parameters: the translations and the
 *             observed points entering the iteration), or lambda > 1e32 (3).  After the stop the remaining launches return at once.
 *   prepare   ls2fm_bundle_adjust_lm_prepare, ONCE per loop (it synchronises `stream`; not capturable): validates view_start and
 *             obs_point exactly as ls2fm_bundle_adjust_prepare does, and view_constant [V] (uint8, device, required).  In
 *             addition LS2FM_ERR_UNSUPPORTED for n_views > LS2FM_BA_LM_MAX_VIEWS and LS2FM_ERR_INVALID_ARGUMENT for a point seen
 *             twice by one view or min_point_views < 1.  The point -> observations lists and the constant flags are the library's
 *             own copies behind a magic header.  workspace: ls2fm_bundle_adjust_lm_workspace_bytes (negative when refused).
 *   run       ls2fm_bundle_adjust_lm_run: n_iters iterations, six plain launches each and two more after the last, nothing read
 *             back: capturable.  poses [V][12] row-major [R | t] world to camera and points [P][3] are updated in place (an
 *             accepted candidate replaces them; a point no picked view observes keeps its bits).  intrinsic4_host: fx, fy, cx, cy
 *             as 4 HOST doubles.  state [8] (device) is owned by the caller and zero before the first call: lambda, done,
 *             iterations taken, current cost, stop reason, max |g| and max |delta| of the last iteration, its accepted flag --
 *             so 2 calls of 3 and 4 iterations equal 1 call of 7 bit for bit, and a replayed graph continues the loop.
 *             log [n_iters][6] (device): cost entering, candidate cost (NaN when a pivot rejected the step; the cost entering
 *             on a gradient stop), lambda used, accepted (1 / 0; -1 for a row after the stop, whose other words are cost, cost,
 *             lambda, 0, 0), max |g|, max |delta|.  LS2FM_ERR_INVALID_ARGUMENT: n_iters < 1, null buffers, loss outside 0..2,
 *             loss_scale / initial_lambda not positive and finite, negative tolerances, sizes as above; LS2FM_ERR_WORKSPACE: null
 *             workspace.  A workspace that prepare did not fill for these sizes moves nothing and logs NaN.
 */
#define LS2FM_BA_LM_MAX_VIEWS 128
typedef struct {
    int32_t loss;              /* 0 trivial, 1 soft_l1, 2 cauchy */
    double loss_scale, initial_lambda, grad_tol, step_tol;
    int32_t min_point_views;   /* prepare's argument decides; kept here for the record of a loop's options */
} ls2fm_ba_lm_opts;
int64_t ls2fm_bundle_adjust_lm_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs);
int ls2fm_bundle_adjust_lm_prepare(const int32_t* view_start, int32_t n_views, const int32_t* obs_point, int64_t n_obs, int64_t n_points,
                                   const uint8_t* view_constant, int32_t min_point_views, void* workspace, void* stream);
int ls2fm_bundle_adjust_lm_run(double* poses, double* points, const double* obs_uv, int32_t n_views, int64_t n_points, int64_t n_obs,
                               const double* intrinsic4_host, const ls2fm_ba_lm_opts* opts, int32_t n_iters, double* state,
                               double* log, void* workspace, void* stream);

/* THE CAMERA BLOCK (additions, the library stays ABI 13): the same loop with the shared camera's LS2FM_CAMERA_PARAMS = 12 words
 * c = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) as a 12-parameter block beside the poses and the points.  All arithmetic fp64,
 * every sum in a fixed order, no floating-point atomics.  tests/ba_lm_camera_restate.py repeats every rule in numpy, by two routes.
 *   model     x_c = R X + t ; x = X_c / Z_c, y = Y_c / Z_c (plain divisions) ; (xd, yd) by THE DISTORTION RULE in fp64 ;
 *             r = (fx xd + cx - u, fy yd + cy - v) with (u, v) the key point IN THE PHOTOGRAPH AS TAKEN.  Loss and IRLS weight as above.
 *   Jacobians J_proj = diag(fx, fy) J_dist [[1/z, 0, -x/z], [0, 1/z, -y/z]], J_dist the rule's Jacobian; J_c and J_p from J_proj as
 *             above.  J_k (2 x 12) by columns: fx (xd, 0) ; fy (0, yd) ; cx (1, 0) ; cy (0, 1) ; k1..k3 (fx x, fy y) r2^j / den ;
 *             k4..k6 -(fx x, fy y) rad r2^j / den ; p1 (fx 2xy, fy (r2 + 2y^2)) ; p2 (fx (r2 + 2x^2), fy 2xy).
 *   words     refine_mask has 12 bits, bit k = word k moves.  An unrefined word has a zero column of J_k; its row and column of the
 *             camera block are the identity's with right-hand side 0 (a constant view's rule, per word).  tie_focal (needs bit 0
 *             set and bit 1 clear): the fx column is col_fx + aspect col_fy, and after an update fy = aspect fx, rounded once;
 *             aspect = fy / fx is formed ONCE by the caller when the loop is built.
 *   system    per observation G += w J_k^T J_k, g_k += w J_k^T r, H_i += w J_c^T J_k (6 x 12, per view), Y_p += w J_k^T J_p (12 x 3,
 *             per point, in the point's list order).  The camera block is damped as ONE 12-block: C* = C + lambda diag(max(C_kk,
 *             1e-12 max_k C_kk)).  The reduced system has 6 V + 12 rows, the camera last:
 *                 S_ik = H_i - sum_{o in view i} w_o J_c,o^T J_p,o V_p*^-1 Y_p^T       S_kk = C* - sum_p Y_p V_p*^-1 Y_p^T
 *                 b_k  = -(g_k - sum_p Y_p V_p*^-1 g_p)      delta_p = -V_p*^-1 (g_p + sum_o W_o^T delta_c[view(o)] + Y_p^T delta_k)
 *             The sums over p are formed as sums over the observations (sum_p Y_p V_p*^-1 Y_p^T = sum_o J_k,o^T F_o with F_o = w_o
 *             J_p,o V_p*^-1 Y_p^T), per view in list order, the views added in view order.  The camera's rows are two more
 *             6-column panels of the same Cholesky: V <= LS2FM_BA_LM_MAX_VIEWS - 2 = 126, LS2FM_ERR_UNSUPPORTED above.
 *   decision  unchanged (strict cost decrease, pivot failure, the lambda rule), with: max |g| includes the refined g_k; max |delta|
 *             includes |delta_k| / (1 + |c_k|) per refined word (a focal length of 1000 px must not loosen the step test of points
 *             of size 1); max |parameter| unchanged.  The candidate camera is accepted or rejected with the poses and points.
 *   run       ls2fm_bundle_adjust_lm_run_camera: prepare is shared (ls2fm_bundle_adjust_lm_prepare on the larger workspace of
 *             ls2fm_bundle_adjust_lm_camera_workspace_bytes, which holds the pinhole layout first).  THE CALLER MUST ALLOCATE THAT
 *             LARGER SIZE: prepare does not know the allocation, its header records V, P and n only, and a workspace of
 *             ls2fm_bundle_adjust_lm_workspace_bytes passed here is written past its end.  camera [12] is DEVICE state,
 *             updated in place like poses: split calls continue bit for bit, a captured call replays, nothing is read back.  Seven
 *             launches per iteration (the border has its own) and two after the last.  refine_mask = 0 is legal: only the residual
 *             model changes.  LS2FM_ERR_INVALID_ARGUMENT: mask bits >= 12, tie_focal with a wrong mask, a non-finite aspect, what
 *             ls2fm_bundle_adjust_lm_run refuses.  A non-finite or zero fx / fy is found on the device: the run moves nothing and
 *             logs NaN, as with an unprepared workspace.
 */
int64_t ls2fm_bundle_adjust_lm_camera_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs);
int ls2fm_bundle_adjust_lm_run_camera(double* poses, double* points, double* camera, const double* obs_uv, int32_t n_views,
                                      int64_t n_points, int64_t n_obs, uint32_t refine_mask, int32_t tie_focal, double aspect,
                                      const ls2fm_ba_lm_opts* opts, int32_t n_iters, double* state, double* log, void* workspace,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Descriptor matching (csrc/match.hip; additions, the library stays ABI 13): the raw matches `colmap exhaustive_matcher` writes
 * into its `matches` table (preparation/main.py:98, read back at :30-37) -- COLMAP's CPU SIFT matcher with its defaults,
 * restated from the published algorithm -- for ALL image pairs in one call.  tests/match_restate.py repeats every rule in numpy.
 *   descriptor 128 unsigned bytes (COLMAP normalises to length 512 and saturates at 255; every byte value 0..255 is served).
 *              desc [N_total][128] holds all images; image v owns rows image_start[v] : image_start[v + 1] (HOST int32
 *              [n_images + 1], from 0, non-decreasing).  pairs [n_pairs][2] (HOST int32): image a (first) and image b (second).
 *   dot(i, j)  the integer inner product of descriptor i of a and descriptor j of b, exact (<= 128 * 255^2 = 8 323 200 < 2^24).
 *   one way    row i over all j in increasing j: best = the largest dot, best_j = the LOWEST j that attains it (COLMAP's strict
 *              >), second = the second largest of the multiset (a tie for the maximum makes second == best); both start at 0,
 *              and a row whose best is 0 has no match (its best_j is reported as -1).
 *   thresholds angle(d) = acos(min(d / 262144, 1)).  Row i proposes best_j unless angle(best) > max_distance or
 *              angle(best) >= max_ratio * angle(second).  COLMAP's defaults: max_ratio 0.8, max_distance 0.7.  Both comparisons
 *              are evaluated in fp64 from the two integers alone (COLMAP evaluates them in fp32: a decision can differ only where
 *              the two sides are within fp32 rounding of each other).
 *   other way  the same rule on the transposed products (rows = descriptors of b, columns = descriptors of a).
 *   cross check (cross_check != 0, COLMAP's default): (i, j) is a match iff i proposes j and j proposes i; 0: the proposals of a.
 *   order      the matches of a pair in increasing i.  At most LS2FM_MATCH_MAX_DESCRIPTORS per image (COLMAP's
 *              max_num_matches); an image with more: LS2FM_ERR_UNSUPPORTED.  Images without descriptors and pairs without a
 *              match are legal and give empty results.  Not restated: guided matching (the two-view geometry is csrc/two_view.hip's).
 *   outputs    (device, int32; sizes follow from the host arrays) with first(p) = sum over q < p of n_a(q) and
 *              rows(p) = sum over q < p of (n_a(q) + n_b(q)):
 *              match_index [sum n_a]: entry first(p) + i = the j matched to row i of pair p's first image, or -1;
 *              num_matches [n_pairs];
 *              best / best_j / second [sum (n_a + n_b)] (each may be NULL): the raw integers of both directions, a -> b at
 *              rows(p) + i (i < n_a, best_j indexes b), b -> a at rows(p) + n_a + j (j < n_b, best_j indexes a).
 *              The compacted [M][2] lists are ls2fm.match's (one nonzero over match_index).
 *   call       asynchronous on `stream`, nothing is read back from the device; the two small tables built from image_start and
 *              pairs are copied from the host inside the call.  desc and workspace must be 16-byte aligned.  Every bit of a
 *              pair's result depends on its own descriptors and the thresholds only: a batch equals the single-pair calls and
 *              a rerun bit for bit (the products are exact integers, the top-2 merges are order independent, the only atomics
 *              are the integer counts).
 *   refusals   nothing enqueued: LS2FM_ERR_INVALID_ARGUMENT for NULL image_start / pairs / desc / match_index / num_matches,
 *              n_images < 1, n_pairs < 0, image_start not rising from 0, a pair index outside [0, n_images), thresholds that are
 *              negative or not finite, a misaligned desc; LS2FM_ERR_UNSUPPORTED for an image above the cap or totals beyond
 *              int32; LS2FM_ERR_WORKSPACE for a NULL or misaligned workspace.  The size query refuses the same way (negative).
 */
#define LS2FM_MATCH_MAX_DESCRIPTORS 32768

int64_t ls2fm_match_descriptors_workspace_bytes(const int32_t* image_start, int32_t n_images, const int32_t* pairs, int32_t n_pairs);
int ls2fm_match_descriptors(const uint8_t* desc, const int32_t* image_start, int32_t n_images, const int32_t* pairs, int32_t n_pairs,
                            double max_ratio, double max_distance, int32_t cross_check, int32_t* match_index, int32_t* num_matches,
                            int32_t* best, int32_t* best_j, int32_t* second, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SIFT feature extraction (csrc/sift.hip; additions, the library stays ABI 13 -- its ABI number is pinned by tests that hold for
 * every addition so far): what `colmap feature_extractor` writes into its `keypoints` and `descriptors` tables
 * (preparation/main.py:91) -- VLFeat-style DoG SIFT with COLMAP's default options, restated from the published algorithm --
 * for all views of a call.  tests/sift_restate.py repeats every rule in numpy (float32 and float64); no bit parity with COLMAP or
 * OpenCV is claimed.  Not restated: affine shape, DSP-SIFT, guided matching.
 *
 *   input       one grey image per view, float32 in [0, 1], H x W >= 16 x 16 and <= 8192 x 8192, sizes free inside one call;
 *               view v starts at pixels[image_offset[v]], rows contiguous.  (uint8 / 255 and RGB by Rec.709 weights
 *               0.2126 / 0.7152 / 0.0722 are ls2fm.features' host-side conversions.)
 *   scale space first_octave -1 (default): the base image is the input up-sampled 2x, out(2y, 2x) = in(y, x), odd columns the mean
 *               of the two neighbours, then odd rows likewise, the last row and column repeated; 0: the input itself.
 *               octave_resolution S = 3 (other values: LS2FM_ERR_UNSUPPORTED); levels s = -1 .. S + 1 (6 Gaussian, 5 DoG) with
 *               blur sigma_s = sigma_0 2^(s/S), sigma_0 = 1.6 * 2^(1/S), in octave pixels; the input's nominal blur is 0.5
 *               (1.0 after the up-sampling).  Level -1 of the first octave is the base blurred by sqrt(sigma_-1^2 - nominal^2),
 *               every further level the previous one blurred by sqrt(sigma_s^2 - sigma_(s-1)^2): separable, taps
 *               exp(-k^2 / 2 sigma^2) for |k| <= ceil(4 sigma), normalised in double and rounded to float once, rows then
 *               columns, edge replication, taps summed from -r to r with one rounded multiply and one rounded add each.
 *               DoG d = level d + 1 - level d  (d = 0 .. 4, its scale s = d - 1).
 *               The next octave (at most num_octaves = 4, fewer when a side would drop below 8) is every second pixel
 *               (0, 2, ...; floor(w / 2) of them) of the level whose blur is twice the first level's: the S-th level above the
 *               first, s = S - 1, so the new first level needs no further blur.
 *   detection   a candidate is a strict 3 x 3 x 3 extremum of the DoG (d = 1 .. 3, 1 <= x <= w - 2, 1 <= y <= h - 2) with
 *               |v| > 0.8 peak_threshold (default 0.02 / S).  At most 5 rounds of the 3-D quadratic fit (central differences,
 *               offset b = -H^-1 g by the adjugate, b = 0 when det H = 0): after a fit the cell moves by one pixel along x
 *               (y) when b exceeds 0.6 in magnitude and the step stays in 1 .. w - 2 (1 .. h - 2); the fifth fit is used where
 *               it stands.  Accepted when |b_x|, |b_y|, |b_s| < 1.5; |v + g.b / 2| > peak_threshold; Dxx Dyy - Dxy^2 > 0 and
 *               (Dxx + Dyy)^2 r < (r + 1)^2 (Dxx Dyy - Dxy^2) with r = edge_threshold (default 10); 0 <= x <= w - 1 and
 *               0 <= y <= h - 1; and the nearest level floor(s + 1/2) is one of 0 .. S - 1 (the refined scale is inside the
 *               octave).
 *   orientation at the nearest level; gradients by central differences on 1 .. w - 2 / 1 .. h - 2; window exp(-r^2 / 2 sw^2) with
 *               sw = 1.5 sigma, support W = max(floor(3 sw), 1) pixels around the nearest pixel, samples with
 *               r^2 >= W^2 + 0.6 skipped; 36 bins, each sample split linearly between the two nearest bin centres; six
 *               circular passes of (h[i-1] + h[i] + h[i+1]) / 3; peaks h[i] > 0.8 max, > both neighbours, refined by the
 *               parabola; the first max_num_orientations (default 2, at most 2) in bin order.  upright != 0: one row, angle 0.
 *   descriptor  4 x 4 spatial bins of width 3 sigma, 8 orientation bins, Gaussian window of 2 bins, support
 *               floor(sqrt(2) * 3 sigma * 5 / 2 + 1/2), trilinear accumulation; L2-normalise, clamp at 0.2, L2-normalise;
 *               then LS2FM_SIFT_L1_ROOT (COLMAP's default: v / sum v, square root) or LS2FM_SIFT_L2; byte = min(255,
 *               floor(512 v + 1/2)).  Stored in the UBC bin order COLMAP stores: VLFeat's index 8 (4 by + bx) + t goes to
 *               8 (4 by + bx) + (8 - t) mod 8.  Histogram bins (here and in the orientation step) are summed exactly, in
 *               2^-40 fixed point with integer adds, and rounded to float once: no floating-point atomic, no order dependence.
 *   order, cap  rows of a view in rising (octave, level, y cell, x cell, orientation index), the cell being the extremum's;
 *               above max_num_features (default 8192, at most LS2FM_MATCH_MAX_DESCRIPTORS) the rows of largest scale are kept,
 *               ties by that order, and the kept rows stay in that order.  A view's rows depend on its own pixels only: the
 *               same bits from a rerun, from any batch around it and from any chunking.
 *   output      keypoints [n_images * max_num_features][4] = x, y, scale, orientation in input pixels with the centre of the
 *               first pixel at (0.5, 0.5) (COLMAP); descriptors [n_images * max_num_features][128] uint8; the rows of view v
 *               start at v * max_num_features; counts [n_images].  counts[v] = -1: the view had more than 32768 accepted
 *               extrema (min(32768, base pixels / 4) for small views) and its rows are not valid.  A constant image gives 0.
 *   workspace   caller-owned, 256-byte aligned, ls2fm_sift_workspace_bytes; the views of a call are processed in chunks whose
 *               workspace stays below max_workspace_bytes (0: 2 GiB; a chunk holds at least one view), so the size is bounded
 *               by the largest chunk, not by the call.  debug_levels (device, n_images must be 1, NULL otherwise): receives the
 *               Gaussian levels, octave after octave, 6 planes each.  debug_keys (device, NULL otherwise)
 *               [n_images * max_num_features][2]: per output row the sort key octave << 30 | level << 28 | y cell << 14 | x cell
 *               and the orientation index.
 *   refusals    nothing enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL array, n_images < 1, a side below 16, an option outside
 *               its range; LS2FM_ERR_UNSUPPORTED for a side above 8192, octave_resolution != 3, num_octaves > 4,
 *               max_num_orientations > 2, max_num_features > LS2FM_MATCH_MAX_DESCRIPTORS; LS2FM_ERR_WORKSPACE for a NULL or
 *               misaligned workspace.
 */
#define LS2FM_SIFT_L1_ROOT 0
#define LS2FM_SIFT_L2 1
typedef struct ls2fm_sift_opts {
    int32_t first_octave;            /* -1 (default) or 0 */
    int32_t num_octaves;             /* 4 */
    int32_t octave_resolution;       /* 3 */
    int32_t max_num_features;        /* 8192 */
    int32_t max_num_orientations;    /* 2 */
    int32_t upright;                 /* 0 */
    int32_t normalization;           /* LS2FM_SIFT_L1_ROOT */
    int32_t reserved;
    double peak_threshold;           /* 0.02 / 3 */
    double edge_threshold;           /* 10 */
    int64_t max_workspace_bytes;     /* 0: 2 GiB */
    float* debug_levels;             /* NULL */
    int32_t* debug_keys;             /* NULL */
} ls2fm_sift_opts;
int64_t ls2fm_sift_workspace_bytes(const int32_t* heights, const int32_t* widths, int32_t n_images, const ls2fm_sift_opts* opts);
int ls2fm_sift_extract(const float* pixels, const int64_t* image_offset, const int32_t* heights, const int32_t* widths, int32_t n_images,
                       const ls2fm_sift_opts* opts, float* keypoints, uint8_t* descriptors, int32_t* counts, void* workspace,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Feature tracks and multi-view triangulation (csrc/tracks.hip; additions, the library stays ABI 13): what the reference keeps in
 * Point3DSet.add_point3d / Camera.idx2d_to_3d, filled pair by pair with cv2.triangulatePoints (pipelines/Registration_Trad.py:183-215,
 * Initialization_Trad.py:97), for all views of a call.  tests/tracks_restate.py repeats every rule in numpy.
 *
 * ls2fm_track_labels: connected components of the match graph.  Nodes are the key points of all views, node image_start[v] + k for
 *   key point k of view v (image_start int32 [n_images + 1], rising from 0 to n_nodes: the caller guarantees it); edges int32
 *   [n_edges][2] are node pairs in any order.  labels int32 [n_nodes]: the smallest node id of the node's component -- the rule and
 *   the union-find of ls2fm_mesh_components (csrc/union_find.h), so labels do not depend on the order of the edges or on
 *   duplicates.  n_edges = 0 writes labels[i] = i.  Three launches, nothing read back.
 *   status int32 [1] (device, may be NULL) is written by the call: 0, or LS2FM_TRACK_EDGE_RANGE when an edge names a node outside
 *   [0, n_nodes), LS2FM_TRACK_EDGE_IMAGE when both ends of an edge lie in one image (or-ed).  Such an edge is checked on the device
 *   before anything is read through it and joins nothing: the call never faults; ls2fm.tracks raises on a non-zero status.
 *   Refused before anything is enqueued (LS2FM_ERR_INVALID_ARGUMENT): a NULL array, n_images < 1, negative counts, n_nodes or
 *   n_edges >= 2^31.
 *   From labels to tracks (ls2fm.tracks.build_tracks, device index operations): a track is a component of >= 2 nodes with at most
 *   one node per image; a component with two nodes in one image is a conflict and is dropped whole (the OpenMVG / hloc rule; COLMAP's
 *   correspondence graph would keep such a component and split it while triangulating).  Tracks in rising label order, the
 *   observations of a track in rising node id (so in rising view).
 *
 * ls2fm_triangulate_tracks: one robust N-view triangulation per track, all geometry in fp64 in normalised image coordinates.
 *   poses [n_views][3][4] world-to-camera P = [R | t]; intrinsics [n_views][4] = fx, fy, cx, cy; track t owns the observations
 *   [track_start[t], track_start[t + 1]) (int32 [n_tracks + 1], rising from 0 to n_obs, at most LS2FM_TRACK_MAX_OBS each);
 *   obs_view int32 [n_obs]; obs_uv [n_obs][2] pixels.  Of an observation (u, v) of view w and a point X:
 *     x = (u - cx) / fx, y = (v - cy) / fy;  xc = ((R00 X0 + R01 X1) + R02 X2) + t0, yc and the depth zc likewise;
 *     e2 = (fx (xc / zc) + cx - u)^2 + (fy (yc / zc) + cy - v)^2;  INLIER when zc > DBL_EPSILON and e2 <= max_error_px^2.
 *     centre C_k = -((R0k t0 + R1k t1) + R2k t2).  angle(X, w, w') = min(a, pi - a), a = acos of the cosine, clamped to [-1, 1],
 *     between X - C_w and X - C_w' (COLMAP's CalculateTriangulationAngle).
 *   hypotheses  every pair i < j of the track's first LS2FM_TRACK_HYP_OBS observations, numbered lexicographically
 *               q = i (2 m - i - 1) / 2 + (j - i - 1), m = min(n, 64): ls2fm_triangulate's 4 x 4 one-sided-Jacobi DLT of the two
 *               normalised observations, X = h[0..2] / h[3].  Dropped when X is not finite, when its depth in either view is <=
 *               DBL_EPSILON, or when angle(X, view i, view j) is not >= min_tri_angle (a NaN angle drops it).
 *   scoring     the inliers of X among ALL observations of the track, an exact integer.  A count of 0 does not compete.
 *   selection   the 64-bit max of count << 32 | (2^32 - 1 - q): the most inliers, then the lowest pair (integer atomics only).
 *   local optimisation  from the best X with count c, at most 10 times while c >= 2: N = sum over the inliers of r r^T for their two
 *               rows x P[2] - P[0] and y P[2] - P[1], each scaled to unit length; the observations are dealt to 8 lanes (number k of
 *               the track to lane k mod 8), a lane adds its own in rising order, and the lanes are summed by the butterfly 4, 2, 1:
 *               a fixed order.  The eigenvector of N's smallest eigenvalue by cyclic Jacobi (relative_pose's routine at size 4; the
 *               lower index among equal eigenvalues), X' = v[0..2] / v[3].  Stop when X' is not finite or counts fewer than c;
 *               otherwise X = X', c = its count, and stop when no observation changed sides.
 *   acceptance  success = c >= 2, every inlier in front (the inlier rule holds it) and the LARGEST angle(X, ., .) over the pairs of
 *               the first 64 inliers >= min_tri_angle.
 *   outputs     X [n_tracks][3] (zero without success), inliers uint8 [n_obs] and num_inliers (of the final X, also without success),
 *               success, tri_angle (that largest angle in radians; 0 below two inliers), mean_error_px (mean of sqrt(e2) over the
 *               inliers; 0 without one), best_pair (q of the selected hypothesis, -1 when none survived; then everything is 0).
 *               Every bit of a track's outputs depends on the track's own observations, their views and the options only.
 *   deviations  COLMAP's estimator scores by angular error and samples long tracks at random; this one scores by pixel error and
 *               is exhaustive over the first 64 observations, so it is deterministic without a seed.
 *   status int32 [1] (device, may be NULL): 0, or LS2FM_TRACK_BAD_START (a track whose extent is not inside [0, n_obs], runs
 *   backwards or exceeds LS2FM_TRACK_MAX_OBS: treated as empty), LS2FM_TRACK_BAD_VIEW (an obs_view outside [0, n_views): never an
 *   inlier, its hypotheses dropped), or-ed.  Checked on the device before use: the call never faults.
 *   Nothing is read back and the launch shapes depend on the counts only: the call can be captured into a graph.
 *   Refused before any launch: LS2FM_ERR_INVALID_ARGUMENT for a NULL array, n_views < 1, negative counts, n_tracks or n_obs >= 2^31,
 *   max_error_px not finite or <= 0, min_tri_angle_deg not in [0, 90]; LS2FM_ERR_WORKSPACE for a NULL workspace.
 */
#define LS2FM_TRACK_HYP_OBS 64
#define LS2FM_TRACK_MAX_OBS 4096
#define LS2FM_TRACK_EDGE_RANGE 1
#define LS2FM_TRACK_EDGE_IMAGE 2
#define LS2FM_TRACK_BAD_START 1
#define LS2FM_TRACK_BAD_VIEW 2
int ls2fm_track_labels(const int32_t* image_start, int32_t n_images, int64_t n_nodes, const int32_t* edges, int64_t n_edges,
                       int32_t* labels, int32_t* status, void* stream);
int64_t ls2fm_triangulate_tracks_workspace_bytes(int64_t n_tracks, int32_t n_views);
int ls2fm_triangulate_tracks(const double* poses, const double* intrinsics, int32_t n_views, const int32_t* track_start,
                             int64_t n_tracks, const int32_t* obs_view, const double* obs_uv, int64_t n_obs, double max_error_px,
                             double min_tri_angle_deg, double* X, uint8_t* inliers, int32_t* num_inliers, int32_t* success,
                             double* tri_angle, double* mean_error_px, int32_t* best_pair, int32_t* status, void* workspace,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * The incremental mapper's two per-step device calls (csrc/mapper.hip behind ls2fm.mapper; additions, the library stays ABI 13): the
 * next-view score that COLMAP's IncrementalMapper::FindNextImages ranks candidates by, and the upkeep of the observation and point
 * state that its CompleteTracks / FilterPoints do one point at a time.  The reference spends one PnP RANSAC per candidate view for
 * the former and keeps the latter in Python lists (pipelines/LevelS2fM.py:247-281, Registration_Trad.py:183-215).
 * tests/mapper_restate.py repeats every rule in numpy.  The track table (track_start, obs_view, obs_uv), poses, intrinsics, the
 * centre, the pixel error e2, the depth zc and angle(X, w, w') are those of ls2fm_triangulate_tracks above (csrc/track_geom.h).
 * Both calls: take a stream and read nothing back; write their status word; use no floating-point atomic (lanes meet in 64-bit
 * integer OR / MAX and in plain stores of one value), so the results do not depend on the launch order and a rerun repeats every
 * bit; launch shapes depend on the counts only, so they can be captured into a graph.  An observation o belongs to the track whose
 * extent holds it, found by bisection over track_start (the last t with track_start[t] <= o; a well-formed table rises), and to
 * none when that track's extent is malformed or does not hold o.  In a malformed table, which the status word reports, an
 * observation may so be left without a track; nothing is ever read outside the arrays.
 *
 * ls2fm_view_scores: COLMAP's VisibilityPyramid score of every view, in one call.
 *   obs_keep uint8 [n_obs], track_valid uint8 [n_tracks], registered uint8 [n_views] (non-zero = true); image_size fp64
 *   [n_views][2] = (W, H) of every view, which the caller guarantees positive and finite.
 *   seen        track t is SEEN iff track_valid[t] and one of its observations o has obs_keep[o] and registered[obs_view[o]].
 *   counting    observation o COUNTS iff its track is seen and its own view is not registered.
 *   num_visible int32 [n_views]: the counting observations of the view (what ls2fm.tracks.visible_points counts).
 *   cells       of a counting observation (x, y) of view v: q = (64.0 * x) / W, cx = 63 when q >= 63, floor(q) when q > 0, else 0
 *               (so pixels left of, on or beyond the borders land in the border cells); cy from y and H likewise.  An
 *               observation with a non-finite x or y is counted in num_visible, marks no cell and sets LS2FM_MAPPER_BAD_PIXEL.
 *   levels      l = 1 .. 6; level l has 2^l x 2^l cells, level 6 is the 64 x 64 grid of (cx, cy); a coarser cell is occupied iff
 *               one of its four children is.
 *   score       int64 [n_views]: sum over l of 4^l x (occupied cells of level l): a cell weighs as many as its level has cells.
 *               One observation scores 4 + 16 + 64 + 256 + 1024 + 4096 = 5460, every cell occupied LS2FM_VIEW_SCORE_MAX
 *               = sum 16^l = 17 895 696.  A registered view has no counting observation: score 0, num_visible 0.
 *   Three launches after the memsets: the seen flags (one lane per observation, its track by bisection), a 4096-bit occupancy mask
 *   per view joined with 64-bit OR atomics, and one wave per view that folds the mask through the levels with shifts, lane
 *   exchanges and popcounts.
 *   status int32 [1] (device, may be NULL): 0, or LS2FM_MAPPER_BAD_START (a track whose extent is not inside [0, n_obs], runs
 *   backwards or exceeds LS2FM_TRACK_MAX_OBS: treated as empty), LS2FM_MAPPER_BAD_VIEW (an obs_view outside [0, n_views): the
 *   observation belongs to no track), LS2FM_MAPPER_BAD_PIXEL, or-ed.  Checked on the device before use: the call never faults.
 *   Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL array, n_views < 1, negative counts, n_tracks or
 *   n_obs >= 2^31; LS2FM_ERR_WORKSPACE for a NULL workspace.
 *
 * ls2fm_update_observations: holds obs_keep / track_valid to the current poses and points, in one call.
 *   X fp64 [n_tracks][3]; track_valid_in uint8 [n_tracks] (may be the array track_valid is written to).
 *   kept        obs_keep[o] = 1 iff o's track t has track_valid_in[t], registered[obs_view[o]], zc > DBL_EPSILON of X[t] in that view
 *               (the "in front" of the triangulation's inlier rule) and e2 <= max_error_px^2; all in fp64, a NaN keeps nothing.
 *               One rule completes tracks into newly registered views and filters what drifted (COLMAP's complete and filter steps
 *               share the threshold).  The pose of a view that is not registered is never read.
 *   num_kept    int32 [n_tracks]: the kept observations of the track.
 *   tri_angle   fp64 [n_tracks]: the LARGEST angle(X[t], w, w') over the pairs of the views of the track's first
 *               LS2FM_TRACK_HYP_OBS kept observations in rising observation order (so rising view), in radians; 0 below two kept;
 *               a NaN angle (X on a centre) does not count: the tri_angle convention of ls2fm_triangulate_tracks.
 *   track_valid = num_kept >= 2 and tri_angle >= min_tri_angle (degrees, converted as min_tri_angle_deg * (pi / 180)).  X is not
 *               changed; obs_keep of a track that ends invalid stays as the rule above gives it.
 *   Five launches after the memset: one lane per observation (its track by bisection) for kept and one per view for the centres;
 *   eight lanes per track that count and pack the views of the first 64 kept; one workgroup's prefix sum of the tracks' pair
 *   counts; one lane per (track, pair) over that flat range, as ls2fm_triangulate_tracks numbers its hypotheses, joining the track's
 *   angle by a 64-bit integer max of the angle's bits (angles are >= 0, so their bits order as they do); one lane per track.
 *   status as above (LS2FM_MAPPER_BAD_START, LS2FM_MAPPER_BAD_VIEW); refused before anything is enqueued as above, and for
 *   max_error_px not finite or <= 0 or min_tri_angle_deg not in [0, 90].
 */
#define LS2FM_MAPPER_BAD_START 1
#define LS2FM_MAPPER_BAD_VIEW 2
#define LS2FM_MAPPER_BAD_PIXEL 4
#define LS2FM_VIEW_SCORE_MAX 17895696
int64_t ls2fm_view_scores_workspace_bytes(int64_t n_tracks, int32_t n_views, int64_t n_obs);
int ls2fm_view_scores(const int32_t* track_start, int64_t n_tracks, const int32_t* obs_view, const double* obs_uv, int64_t n_obs,
                      const uint8_t* obs_keep, const uint8_t* track_valid, const uint8_t* registered, const double* image_size,
                      int32_t n_views, int64_t* score, int32_t* num_visible, int32_t* status, void* workspace, void* stream);
int64_t ls2fm_update_observations_workspace_bytes(int64_t n_tracks, int32_t n_views, int64_t n_obs);
int ls2fm_update_observations(const double* poses, const double* intrinsics, const uint8_t* registered, int32_t n_views,
                              const int32_t* track_start, int64_t n_tracks, const int32_t* obs_view, const double* obs_uv,
                              int64_t n_obs, const double* X, const uint8_t* track_valid_in, double max_error_px,
                              double min_tri_angle_deg, uint8_t* obs_keep, uint8_t* track_valid, int32_t* num_kept, double* tri_angle,
                              int32_t* status, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact nearest neighbours between two point clouds (csrc/point_grid.hip behind ls2fm.metrics; additions, the library stays ABI
 * 13): the primitive of the Chamfer distance of a mesh against ground truth.  The reference ships no evaluation.
 * tests/metrics_restate.py repeats the distance rule in numpy.
 *
 * distance rule  of a query q and a reference r, in fp32: dx = q.x - r.x, dy and dz likewise, d2 = (dx dx + dy dy) + dz dz, every
 *   operation rounded once, none contracted.  r QUALIFIES when d2 <= max_d2 and d2 < +inf.  The neighbour of q is the qualifying
 *   reference of smallest d2, among equal d2 the one of lowest index: a pure function of the two clouds and max_d2, whatever
 *   the grid, the batching of the queries or the order of the visits.  A query without a qualifying reference -- every query
 *   with a NaN or infinite coordinate is one -- gets index -1 and d2 = +inf.  max_d2 = +inf is "no cut-off"; NaN or a negative
 *   max_d2 is refused.
 * grid  origin float [3], cell_size h > 0, inv_cell_size (the caller's fp32 1 / h) and dim int32 [3] describe a uniform grid of
 *   dim[0] dim[1] dim[2] < 2^31 - 1 cells; the cell of p on an axis is clamp(floor((p - origin) * inv_cell_size), 0, dim - 1) in
 *   fp32 (fminf / fmaxf before the conversion, so a NaN lands in a border cell), cell id = (cz dim[1] + cy) dim[0] + cx.  For
 *   exact answers the caller makes origin the per-axis minimum of the references and dim at least that formula's cell of the
 *   per-axis maximum plus one, so that no reference is clamped (ls2fm.metrics.PointGrid does); any other grid is still walked
 *   without a read outside the arrays.
 * build  ref float [n_points][3] (finite: the caller guarantees it) -> cell_start int32 [cells + 1], the exclusive prefix sum of
 *   the cells' point counts, and sorted float [n_points][4], 16-byte aligned: the points in cell order as x, y, z and the BITS of
 *   their int32 index in ref.  Counting and scattering use 32-bit integer atomics, so the order inside a cell may differ between
 *   runs; no result of a query depends on it.  workspace: the size query's bytes (negative: refused sizes).  n_points = 0 zeroes
 *   cell_start.  One memset and five launches, nothing read back.
 * query  queries float [n_queries][3] -> idx int32 [n_queries] (index into ref, or -1), d2 float [n_queries].  One launch, one
 *   query per lane: the query's own cell, then the Chebyshev rings 1, 2, ... around it.  After ring k every unvisited reference is
 *   at least (k - slack) h away, slack = 2^-21 max(dim) covering the two fp32 roundings of the cell assignment, and the walk stops
 *   when min(best d2, max_d2) < ((k - slack) h)^2 (1 - 2^-18), strictly, so that a tied reference of a later ring is still
 *   visited; the factor covers the rounding of d2 itself.  The ring loop runs at most max(dim) + 1 times.  Nothing is read back:
 *   the call can be captured into a graph.  n_queries = 0 returns at once; n_points = 0 fills -1 / +inf without a launch.
 * No floating-point atomic anywhere.  Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL array, a
 * negative count, n_points >= 2^31, a cell size or reciprocal that is not positive and finite, a dim below 1 or 2^31 - 1 cells or
 * more, a misaligned sorted; LS2FM_ERR_WORKSPACE for a NULL workspace.
 */
int64_t ls2fm_point_grid_workspace_bytes(int64_t n_points, int64_t n_cells);
int ls2fm_point_grid_build(const float* ref, int64_t n_points, const float* origin, float cell_size, float inv_cell_size,
                           const int32_t* dim, int32_t* cell_start, float* sorted, void* workspace, void* stream);
int ls2fm_point_grid_query(const float* queries, int64_t n_queries, const float* sorted, const int32_t* cell_start, int64_t n_points,
                           const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, float max_d2, int32_t* idx,
                           float* d2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The k nearest neighbours of a query and the normals of a cloud (csrc/point_grid.hip, csrc/cloud_normals.hip behind
 * ls2fm.metrics.PointGrid.knn and ls2fm.cloud; additions, the library stays ABI 13).  The reference ships none.
 * tests/cloud_restate.py repeats both rules in numpy.
 *
 * K-NEIGHBOUR RULE  under the distance rule and its qualification (d2 <= max_d2 and d2 < +inf, above) the neighbours of a query
 *   are its qualifying references ordered by (d2, index) ascending, the first k of them, 1 <= k <= 32.  idx int32 [n_queries][k]
 *   holds their indices and -1 in the slots without a neighbour, d2 float [n_queries][k] their d2 and +inf in those slots,
 *   count int32 [n_queries] how many slots are filled.  A NaN or infinite query has none.  With skip_own != 0 query t ignores the
 *   reference whose original index is t: the caller promises that the queries are the references in their order, and the call is
 *   refused unless n_queries == n_points; a duplicate of point t at another index stays a neighbour at d2 = 0.  The result is a
 *   pure function of the two clouds, k, max_d2 and the flag: no grid, batch, visiting order or list capacity shows in it.
 * knn  one launch, one query per lane, the rings of the query above with a sorted list of the k best in registers (capacities 8,
 *   16 and 32 are instantiated; the smallest that holds k runs).  After ring r the walk stops when
 *   min(d2 of the k-th entry -- +inf while there are fewer than k --, max_d2) < ring bound of r, strictly, for the reason given
 *   above; the whole-grid exit is unchanged.  Nothing is read back: the call can be captured into a graph.  n_queries = 0 returns
 *   at once; n_points = 0 fills -1 / +inf / 0 without a launch.  Refused as the query refuses, and for k outside 1 .. 32.
 *
 * NORMAL RULE  of points float [n_points][3] and a neighbour list idx int32 [n_queries][k] (k >= 1; rows of the knn above, or any
 *   other list).  Per query, over the n entries with 0 <= idx < n_points in list order (any other entry is no neighbour),
 *   everything in fp64 of the fp32 inputs, every operation rounded once, none contracted:
 *     mean        m = (((p0 + p1) + p2) + ...) / n
 *     covariance  d_j = p_j - m;  C_ab = (((d_0a d_0b + d_1a d_1b) + d_2a d_2b) + ...) / n, the six entries xx xy xz yy yz zz
 *     eigen       the cyclic Jacobi of the symmetric 3 x 3 (pose_math.h's jacobi3_sym: the threshold, sweep cap and rotation
 *                 formulas of jacobi4); lambda_i is the diagonal after it.  The normal is the eigenvector of the smallest
 *                 lambda, the lowest index among equals, divided by its length sqrt((v.x v.x + v.y v.y) + v.z v.z);
 *                 curvature = that lambda / ((lambda_0 + lambda_1) + lambda_2)
 *     n < 3, or a trace (C_xx + C_yy) + C_zz that is zero or NaN: NaN for the normal and the curvature (cov is still C; NaN for
 *                 n = 0)
 *     orientation with toward float [1 or n_queries][3] and queries float [n_queries][3]: the normal is negated when
 *                 (v.x t.x + v.y t.y) + v.z t.z < 0, t = toward - query in fp64 (zero keeps the sign).  Without toward: negated
 *                 when its component of largest magnitude, the lowest axis among equals, is negative.
 *   -> normal double [n_queries][3], curvature double [n_queries], cov double [n_queries][6] (may be NULL).
 * normals  one launch, one query per lane, k gathers from points (twice: mean, covariance); no atomics, no workspace, nothing
 *   read back.  Refused: a NULL array that is needed, a negative count, n_points >= 2^31, k < 1, toward without queries or with
 *   n_toward neither 1 nor n_queries.
 */
int ls2fm_point_grid_knn(const float* queries, int64_t n_queries, const float* sorted, const int32_t* cell_start, int64_t n_points,
                         const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, int32_t k, float max_d2,
                         int32_t skip_own, int32_t* idx, float* d2, int32_t* count, void* stream);
int ls2fm_cloud_normals(const float* points, int64_t n_points, const int32_t* idx, int64_t n_queries, int32_t k, const float* queries,
                        const float* toward, int64_t n_toward, double* normal, double* curvature, double* cov, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The implicit surface of an oriented point cloud on a dense lattice (csrc/cloud_implicit.hip behind ls2fm.cloud_mesh; an
 * addition, the library stays ABI 13): what marching cubes needs to mesh a scan, a filtered MVS cloud or the mapper's points.
 * The reference ships none.  tests/cloud_mesh_restate.py repeats the rule in numpy.
 *
 * THE IMPLICIT RULE  of points float [n_points][3] (finite: the caller's promise, as for ls2fm_point_grid_build), normals float
 *   [n_points][3], a point grid built over the points, a lattice nx x ny x nz with origin float [3] and voxel, k in 1 .. 32,
 *   max_d2 finite and > 0 (+inf is refused: the weight needs it) and min_neighbors >= 1.  Lattice point i sits at
 *   X[a] = fl32(fl32((float) i[a] * voxel) + origin[a]), the expression of ls2fm_tsdf_integrate and ls2fm_marching_cubes_emit;
 *   axis 2 is the fastest.  Its neighbours are the list of the K-NEIGHBOUR RULE for the query X with k and max_d2, no skip_own:
 *   entries (d2_j, i_j), j = 0 .. n - 1, in list order.  Then in fp64 of the fp32 inputs, every operation rounded once, none
 *   contracted, P = points[i_j], N = normals[i_j]:
 *     t_j = 1 - (double) d2_j / (double) max_d2
 *     w_j = (t_j t_j) t_j
 *     s_j = (N.x (X.x - P.x) + N.y (X.y - P.y)) + N.z (X.z - P.z)
 *     den = ((w_0 + w_1) + w_2) + ...            num = ((w_0 s_0 + w_1 s_1) + w_2 s_2) + ...     both start from their first term
 *     value   = fl32(num / den)  when n >= min_neighbors and den > 0, NaN otherwise
 *     support = fl32(den)        (0 when n = 0)
 *   A non-finite normal makes value NaN at every lattice point that lists its point (ls2fm.cloud_mesh removes such points
 *   first); a neighbour at exactly d2 == max_d2 has weight 0; the value is positive on the side the normals point to, the sign of
 *   the FUSION RULE, so marching cubes' faces come out oriented like ls2fm.fusion.extract's.  value and support are float
 *   [nx][ny][nz]; support may be NULL.  The value is a pure function of the cloud, the normals, the lattice, k, max_d2 and
 *   min_neighbors: neither the grid's cell size, the brick nor the order of the visits shows in it.
 * implicit  one launch, one lane per lattice point: the lane forms X, runs the k-nearest walk with the list in registers
 *   (capacities 8, 16, 32; the smallest that holds k) and sums over the finished list.  No atomics, no workspace, nothing read
 *   back: the call can be captured.  n_points = 0 fills NaN / 0 without a walk.  ls2fm_cloud_implicit_plan is the same call
 *   with the launch plan chosen: brick 0 is LS2FM_CLOUD_IMPLICIT_BRICK0_X x _Y x _Z lattice points per workgroup (a wave along
 *   axis 2), brick 1 is ..._BRICK1_X x _Y x _Z (a wave a cube of 4 x 4 x 4); with empty_test = 1 a workgroup whose brick, grown
 *   by the radius, overlaps no occupied grid cell writes NaN / 0 without walking.  No plan shows in a bit of the result;
 *   ls2fm_cloud_implicit runs LS2FM_CLOUD_IMPLICIT_BRICK and LS2FM_CLOUD_IMPLICIT_EMPTY_TEST, the measured fastest.
 *   Refused before anything is enqueued, LS2FM_ERR_INVALID_ARGUMENT: a NULL array that is needed, a negative count, n_points >=
 *   2^31, a lattice side below 1 or above 2^24 or a lattice of 2^31 points or more, a voxel that is not positive and finite, a
 *   non-finite origin, k outside 1 .. 32, max_d2 not finite or <= 0, min_neighbors < 1, a plan that is neither 0 nor 1, and
 *   what ls2fm_point_grid_knn refuses of the grid.
 */
#define LS2FM_CLOUD_IMPLICIT_BRICK0_X 2
#define LS2FM_CLOUD_IMPLICIT_BRICK0_Y 2
#define LS2FM_CLOUD_IMPLICIT_BRICK0_Z 64
#define LS2FM_CLOUD_IMPLICIT_BRICK1_X 8
#define LS2FM_CLOUD_IMPLICIT_BRICK1_Y 8
#define LS2FM_CLOUD_IMPLICIT_BRICK1_Z 4
#define LS2FM_CLOUD_IMPLICIT_BRICK 1
#define LS2FM_CLOUD_IMPLICIT_EMPTY_TEST 1
int ls2fm_cloud_implicit(const float* points, const float* normals, int64_t n_points, const float* sorted, const int32_t* cell_start,
                         const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, int64_t nx, int64_t ny, int64_t nz,
                         const float* lattice_origin, float voxel, int32_t k, float max_d2, int32_t min_neighbors, float* value,
                         float* support, void* stream);
int ls2fm_cloud_implicit_plan(const float* points, const float* normals, int64_t n_points, const float* sorted, const int32_t* cell_start,
                              const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, int64_t nx, int64_t ny,
                              int64_t nz, const float* lattice_origin, float voxel, int32_t k, float max_d2, int32_t min_neighbors,
                              int32_t brick, int32_t empty_test, float* value, float* support, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Screened Poisson reconstruction of an oriented point cloud on the dense lattice (csrc/poisson.hip behind
 * ls2fm.cloud_mesh.poisson_from_cloud; additions, the library stays ABI 13): a global solve, so holes close by one stated rule
 * where the implicit rule above leaves them open.  The reference ships none.  tests/poisson_restate.py repeats the rule in numpy.
 *
 * THE POISSON RULE  The unknown chi lives on the lattice n0 x n1 x n2 (every side >= 2, axis 2 fastest), lattice point i at
 *   fl32(fl32((float) i * voxel) + origin).  All lattice arithmetic is fp32; every operation below is ONE rounded operation in
 *   the stated order, none contracted, division correctly rounded.  fl() is that rounding.
 *   1 splat   For point P with normal N (fp32), per axis a: u = fl(fl(P_a - origin_a) / voxel), i_a = floor(u), f_a = u - i_a
 *     (exact).  The point takes part when 0 <= u < n_a - 1 on every axis and P and N are finite; otherwise it adds nothing.  The
 *     weight at corner (dx, dy, dz) of its cell is w = fl(fl(wx wy) wz), w_a = f_a at the upper corner and fl(1 - f_a) at the
 *     lower.  The corner receives w into the density W and w N_a into V_a, each term as rint((double) w (double) N_a 2^32), an
 *     int64 (the product is exact in fp64; the conversion goes through the double's mantissa and is rint while the term stays
 *     below 2^51, i. e. |N_a| < 2^19), added with 64-bit INTEGER atomics into four accumulators per lattice point: no order
 *     shows.  Then V_a = (float) ((double) sum 2^-32), W likewise.  Exactness needs, per lattice point, sum |w N_a| < 2^30: with
 *     unit normals (ls2fm.cloud_mesh normalises them) that is a bound of 2^30 on the points around one lattice point.
 *   2 right-hand side   g(i, i + e_a) = fl(0.5 fl(V_a[i] + V_a[i + e_a])) on every lattice edge;  t_a = fl(g(i - e_a, i) -
 *     g(i, i + e_a)), a missing edge counted as 0;  b_i = fl(fl(t_0 + t_1) + t_2).  These are the normal equations of
 *     sum over edges (chi_j - chi_i - g_ij)^2 + screen sum_i W_i chi_i^2: a graph Laplacian with natural boundaries plus a
 *     lumped screening term.  Summed, they give sum W_i chi_i = 0: the surface is the ZERO level, no isovalue is reduced;
 *     outward normals make chi positive outside, the sign of the FUSION RULE.
 *   3 operator at level l   s = 4^-l (exact), a = screen (fp32).  N_i is the sum of the existing neighbours in the order -0, +0,
 *     -1, +1, -2, +2, starting from the first that exists; deg_i their count;  D_i = fl(fl(s deg_i) + fl(a W_i)).
 *     smoother: red-black Gauss-Seidel in place, colour (i0 + i1 + i2) & 1 == 0 first:  chi_i <- fl(fl(b_i + fl(s N_i)) / D_i)
 *     residual: r_i = fl(b_i - fl(fl(s fl(fl(deg_i chi_i) - N_i)) + fl(fl(a W_i) chi_i)))
 *   4 levels   a coarse side is nc = (n + 1) / 2, coarse I on fine 2 I; level l + 1 exists while level l has its smallest side
 *     >= 4 and its largest >= 5.  Prolongation along an axis: even i copies e[i / 2], odd i takes fl(0.5 fl(e[(i - 1) / 2] +
 *     e[min((i + 1) / 2, nc - 1)])); in three dimensions the axes in the order 0, 1, 2; the correction is chi <- fl(chi + P e).
 *     Restriction is its transpose, halved per axis: acc = fl(0.5 r[2 I]), + fl(0.25 r[2 I - 1]) if that point exists, + fl(c
 *     r[2 I + 1]) if that point exists, c = 0.5 when 2 I + 2 == n (the last point of an even side) and 0.25 otherwise; the axes
 *     in the order 0, 1, 2; no renormalisation at the boundary.  W_{l+1} = R W_l by the same restriction.
 *   5 cycle   cycle(l) on the coarsest level is 32 sweeps from the chi it is given; on any other level 2 sweeps, then gamma
 *     times { r; b_{l+1} = R r; chi_{l+1} = 0; cycle(l + 1); chi_l += P chi_{l+1} }, then 2 sweeps.  The solve is `cycles` calls
 *     of cycle(0) from chi = 0: a fixed count, no stopping test, nothing read on the host.
 * ls2fm_poisson_solve  splat -> finish and right-hand side -> W of the levels -> the cycles, launched in a fixed order on `stream`
 *   and capturable; value (chi) and density (W of level 0) are float [nx][ny][nz].  n_points = 0 gives chi = 0 and W = 0.  From
 *   the first level of at most LS2FM_POISSON_TAIL_POINTS points downward one launch of one workgroup runs the whole sub-cycle in
 *   LDS, with the device functions of the per-level kernels: the same bits.  ls2fm_poisson_solve_plan chooses tail_points = 0
 *   (every level by its own launches) or LS2FM_POISSON_TAIL_POINTS; no plan shows in a bit.  The sweep kernel's brick is
 *   LS2FM_POISSON_BRICK_X x _Y x _Z lattice points per workgroup.  The workspace (256-byte aligned,
 *   ls2fm_poisson_workspace_bytes; -1 for a lattice that is refused) holds the accumulators, whose bytes the coarse levels take
 *   over once the finish has read them, and b of level 0.
 *   Refused before anything is enqueued, LS2FM_ERR_INVALID_ARGUMENT: a side below 2 or above 2^24, nx ny or the lattice 2^31
 *   points or more, a voxel that is not positive and finite, a non-finite origin, n_points < 0 or >= 2^31, cycles < 0, gamma
 *   not 1 or 2, screen not finite and positive, tail_points neither 0 nor LS2FM_POISSON_TAIL_POINTS, a NULL array that is
 *   needed, a workspace that is NULL, misaligned or too small.
 * The stages one at a time, with the kernels of the solve (the tests hold each to the restatement): ls2fm_poisson_splat (splat,
 *   finish and right-hand side: V float [3][nx][ny][nz] or NULL, b, density; workspace of 32 bytes a lattice point),
 *   ls2fm_poisson_sweep_colour (one colour of one sweep at scale s, in place), ls2fm_poisson_restrict (coarse = R r of chi, b,
 *   density at scale s; with b and density NULL coarse = R chi; coarse is float [(nx + 1) / 2][(ny + 1) / 2][(nz + 1) / 2]) and
 *   ls2fm_poisson_prolong (chi += P coarse).
 */
#define LS2FM_POISSON_BRICK_X 2
#define LS2FM_POISSON_BRICK_Y 2
#define LS2FM_POISSON_BRICK_Z 128
#define LS2FM_POISSON_TAIL_POINTS 4096
int64_t ls2fm_poisson_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int ls2fm_poisson_solve(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                        const float* origin, float voxel, float screen, int32_t cycles, int32_t gamma, float* value, float* density,
                        void* workspace, int64_t workspace_bytes, void* stream);
int ls2fm_poisson_solve_plan(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                             const float* origin, float voxel, float screen, int32_t cycles, int32_t gamma, int32_t tail_points,
                             float* value, float* density, void* workspace, int64_t workspace_bytes, void* stream);
int ls2fm_poisson_splat(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                        const float* origin, float voxel, float* V, float* b, float* density, void* workspace, int64_t workspace_bytes,
                        void* stream);
int ls2fm_poisson_sweep_colour(float* chi, const float* b, const float* density, int64_t nx, int64_t ny, int64_t nz, float scale,
                               float screen, int32_t colour, void* stream);
int ls2fm_poisson_restrict(const float* chi, const float* b, const float* density, int64_t nx, int64_t ny, int64_t nz, float scale,
                           float screen, float* coarse, void* stream);
int ls2fm_poisson_prolong(float* chi, int64_t nx, int64_t ny, int64_t nz, const float* coarse, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ICP registration of a moving cloud to a fixed one (csrc/icp.hip behind ls2fm.metrics.icp; additions, the library stays ABI
 * 13): the step between the camera alignment and the Chamfer figures of a reconstruction in its own gauge.  The reference ships
 * none.  tests/icp_restate.py repeats the rule in numpy.
 *
 * The fixed cloud is a built point grid (sorted, cell_start, n_dst and the grid description of ls2fm_point_grid_build); the
 * moving cloud is src float [n_src][3].  The transform (s, R, t) lives in the caller's state, double [24]:
 *   [0] s   [1 .. 9] R row-major   [10 .. 12] t   [13] cost of the last accumulate   [14] its pair count   [15] iterations done
 *   [16] status: 0 running, 1 converged, 2 degenerate   [17 .. 23] reserved, written as 0
 * The caller initialises s, R, t and sets [13 .. 23] to 0.  Because the state is the caller's, split calls (iters = a, then
 * iters = b) continue bit for bit like one call of a + b.
 * accumulate  per source point p = (x, y, z), widened to fp64: p'_i = s ((R_i0 x + R_i1 y) + R_i2 z) + t_i, every operation
 *   rounded once in this association, none contracted; p' is then rounded once to fp32 and is the query of the grid walk under
 *   the distance rule and max_d2 (above).  A p' that is not finite has no pair; a source point without a qualifying reference
 *   has no pair.  For a pair (p', q), q the stored fp32 reference and p' the fp32 point, both widened to fp64, the Gauss-Newton
 *   normal equations of the left perturbation xi = (omega, upsilon, lambda), p'' = e^lambda exp([omega]x) p' + upsilon:
 *     point to point (dst_normals NULL)   r = p' - q (three rows),  J = [-[p']x, I, p']
 *     point to plane (dst_normals float [n_dst][3], of the fixed cloud, read at the winner's index n)
 *                                         r = (n.x d.x + n.y d.y) + n.z d.z, d = p' - q (one row),
 *                                         J = [p' x n, n, (n.x p'.x + n.y p'.y) + n.z p'.z],  (p' x n).x = p'.y n.z - p'.z n.y, ...
 *   A pair's term of H_ab is J_0a J_0b, with three rows (J_0a J_0b + J_1a J_1b) + J_2a J_2b; of g_a the same with r in place
 *   of J_.b; of the cost the same with r twice.  The 36 sums: the 28 entries of the upper triangle of H row-major, g (7), the
 *   cost.  No floating-point atomic: a lane adds its own points in index order (point i belongs to lane i mod the launch's
 *   lanes), the lanes of a workgroup are added in the fixed order of the library's workgroup sum, and the workgroups' partial
 *   rows are added in row order.  The launch shape and the rows depend on n_src alone: min(ceil(n_src / 512), 512) workgroups of
 *   512 lanes.  The pair count is an exact integer.  pair_idx int32 [n_src] and pair_d2 float [n_src] (each may be NULL) receive
 *   the winner's index and d2, -1 and +inf without a pair; sums double [36] (may be NULL) the sums of the last accumulate.
 * solve  H delta = -g by Cholesky in fp64, 7 x 7 with with_scale != 0, else the leading 6 x 6 (lambda = 0).  E = exp([omega]x) by
 *   Rodrigues' formula (below |omega|^2 = 1e-30: I + [omega]x), k = 1 + expm1(lambda) (e^lambda, evaluated so that its error scales
 *   with |lambda|; 1 without scale); s <- k s, R <- E R, t <- k (E t) + upsilon, each entry (a b + c d) + e f.
 *   A pivot <= 0, a delta that is not finite or fewer pairs than unknowns: status DEGENERATE, the transform unchanged bit for
 *   bit, the iteration not counted.  Otherwise the update is applied and counted, and max(|omega_i|, |lambda|) <= tol_rot together
 *   with max |upsilon_i| <= tol_trans sets status CONVERGED.
 * Every kernel reads the status first and does nothing once it is not 0: a call on a converged or degenerate state changes
 * nothing, neither the state nor the pair arrays nor sums.  iters >= 1: two launches per iteration (accumulate, solve), iters
 * of them whatever the status becomes.  iters = 0: one accumulate and the reduction of its rows (the solve's kernel, which stops
 * after writing cost, pair count and sums): cost, count and pairs at the state's transform, the transform, the iteration count
 * and the status untouched.  Nothing is read back: the call can be captured into a graph.  n_src = 0 or n_dst = 0: no walk, cost
 * and count 0, status DEGENERATE at once (n_dst = 0 fills the pair arrays with -1 / +inf first).  This takes precedence over
 * iters = 0 leaving the status untouched: an empty side sets DEGENERATE whatever iters is.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL array that is needed, a negative count or one of
 * 2^31 or more, iters < 0 or above LS2FM_ICP_MAX_ITERS, a NaN or negative max_d2, tol_rot or tol_trans, a grid description the
 * query refuses, a misaligned sorted; LS2FM_ERR_WORKSPACE for a NULL workspace (ls2fm_icp_workspace_bytes(n_src) bytes).
 */
#define LS2FM_ICP_MAX_ITERS 65536
int64_t ls2fm_icp_workspace_bytes(int64_t n_src);
int ls2fm_icp_run(const float* src, int64_t n_src, const float* sorted, const int32_t* cell_start, int64_t n_dst, const float* origin,
                  float cell_size, float inv_cell_size, const int32_t* dim, const float* dst_normals, float max_d2, int32_t with_scale,
                  int32_t iters, double tol_rot, double tol_trans, double* state, double* sums, int32_t* pair_idx, float* pair_d2,
                  void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A triangle rasteriser with a z-buffer (csrc/rasterize.hip behind ls2fm.raster; additions, the library stays ABI 13): which
 * faces of a mesh each camera sees, mesh depth maps, per-pixel face ids and barycentrics, and per-vertex mask votes -- the
 * culling step in front of the DTU Chamfer figures.  The reference ships none.  tests/raster_restate.py repeats the rule in numpy.
 *
 * Inputs: verts float [V][3]; faces int32 [F][3]; poses float [N][3][4], world-to-camera [R | t]; intr float [N][4] =
 * (fx, fy, cx, cy), on the device (skew is not modelled); height, width; near > 0.  Pixel (px, py) has its centre at
 * (px + 0.5, py + 0.5).  The RASTERISATION RULE, for one view and one face (a, b, c):
 *   camera point  of a vertex X, in fp32: for row r of the pose, c_r = ((P_r0 X_0 + P_r1 X_1) + P_r2 X_2) + P_r3, every
 *     operation rounded once, none contracted.
 *   projection    u = fx * (c_x / c_z) + cx, v = fy * (c_y / c_z) + cy, each operation one rounded fp32 operation.
 *   usable vertex c_z is finite, c_z >= near, |u| <= 65536 and |v| <= 65536.  A NaN fails every one of these comparisons.
 *   snap          U = (int) rintf(u * 256), V likewise: 8 sub-pixel bits, |U| <= 2^24.  Every integer below stays under 2^52,
 *     so its conversion to double is exact.
 *   drawn face    a face is drawn in a view if and only if its three indices lie in [0, V), all three vertices are usable,
 *     and A = (U_b - U_a)(V_c - V_a) - (V_b - V_a)(U_c - U_a) (int64) is not 0.
 *   no clipping   a face with an unusable vertex is simply not drawn in that view (a stated deviation: marching-cubes
 *     triangles are voxel-sized, so what crosses the near plane is negligible).  No back-face culling: back faces occlude.
 *   coverage      in exact integers.  s = sign(A), P = (256 px + 128, 256 py + 128).  For the edge p -> q,
 *     E_pq(P) = (U_q - U_p)(P_y - V_p) - (V_q - V_p)(P_x - U_p).  w_a = s E_bc, w_b = s E_ca, w_c = s E_ab, so that
 *     w_a + w_b + w_c = s A = |A|.  An edge OWNS its boundary when its normalised direction d = s (U_q - U_p, V_q - V_p) has
 *     d_y > 0, or d_y == 0 and d_x > 0.  The pixel is covered if and only if each w_i > 0, or w_i == 0 and that edge owns its
 *     boundary.  The two triangles on either side of a shared edge traverse it in opposite directions after normalisation, so
 *     exactly one of them takes a pixel centre lying on the edge.
 *   depth         camera z, perspective-correct, in fp64.  Per face r_i = 1.0 / (double) c_z,i.  Per pixel
 *     num = ((double) w_a r_a + (double) w_b r_b) + (double) w_c r_c, z = (float)((double) |A| / num): one division per pixel,
 *     every operation rounded once.  The barycentrics are beta_i = (float)(((double) w_i r_i) / num).
 *   z-test        key = ((uint64) bits(z) << 32) | (uint32) f; the smallest key wins: the nearest depth, among equal depth
 *     bits the lowest face index.  No visiting order, batching or path shows in the result.
 *   empty pixel   face_id = -1, depth = +inf, barycentrics 0.
 *
 * ls2fm_rasterize  -> face_id int32 [N][H][W], depth float [N][H][W], bary float [N][H][W][3] (or NULL), and face_hits int32 [F]
 *   (or NULL; caller-zeroed): face_hits[f] += the pixels face f won, over the N views (32-bit integer atomics: exact, so reruns
 *   agree).  workspace: the uint64 z-buffer, 8 n_views height width bytes, 8-byte aligned (the size query; negative: refused
 *   sizes).  Three launches -- the workspace cleared to all-ones (by a kernel: a captured memset node was seen not to be ordered
 *   with the kernels after it on replay), the raster kernel, the resolve kernel; nothing is read back, nothing is allocated and
 *   no stream is forked, so the call can be captured.  The raster kernel takes one lane per (view, face): it sets
 *   the face up, clips the box of pixel centres inside the face's bounds to the image, and walks the box when it holds at most
 *   LS2FM_RASTER_LANE_PIXELS pixels; the wave then takes its remaining faces one at a time, the set-up broadcast, all 64 lanes
 *   striding the box.  Both paths evaluate the same integer and fp64 expressions per pixel.  Its only atomic is the 64-bit
 *   unsigned minimum on the z-buffer (the key is read first and the atomic skipped when it would not lower it: keys only fall).
 *   The resolve kernel unpacks face_id and depth and recomputes the winner's barycentrics from the rule.  No floating-point
 *   atomic anywhere.  n_views = 0 returns at once; n_faces = 0 fills -1 / +inf (and barycentrics 0).
 * ls2fm_mesh_mask_votes  masks uint8 [N][H][W] -> seen, inside int32 [V] (overwritten).  One lane per vertex, looping over the
 *   views, no atomics; the same camera point, projection and usable rule.  The vertex is IN THE IMAGE when 0 <= u < width and
 *   0 <= v < height, as fp32 comparisons; its pixel is (floor(u), floor(v)).  seen[v] counts the views where the vertex is
 *   usable and in the image, inside[v] those of them whose mask byte is non-zero.  n_verts = 0 returns at once; n_views = 0
 *   writes zeros.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL required array (bary and face_hits are optional;
 * verts and faces are required when n_faces > 0), a negative count, n_faces >= 2^31, height or width outside [1, 32768], a
 * near that is not positive and finite, n_views height width >= 2^40, a workspace that is not 8-byte aligned;
 * LS2FM_ERR_WORKSPACE for a NULL workspace.
 */
#define LS2FM_RASTER_LANE_PIXELS 16   /* a face whose clipped box holds more pixels than this is walked by its whole wave */
int64_t ls2fm_rasterize_workspace_bytes(int32_t n_views, int32_t height, int32_t width);
int ls2fm_rasterize(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* poses, const float* intr,
                    int32_t n_views, int32_t height, int32_t width, float near, int32_t* face_id, float* depth, float* bary,
                    int32_t* face_hits, void* workspace, void* stream);
int ls2fm_mesh_mask_votes(const float* verts, int64_t n_verts, const float* poses, const float* intr, int32_t n_views, int32_t height,
                          int32_t width, float near, const uint8_t* masks, int32_t* seen, int32_t* inside, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image-quality metrics of rendered views against photographs (csrc/image_metrics.hip behind ls2fm.image_metrics; additions, the
 * library stays ABI 13, the number the host tests of earlier additions pin): the squared error behind PSNR, and SSIM over the
 * valid region, per view, in fp64.  The reference has only the training-time PSNR of the sampled rays (pipelines/Camera.py:534).
 * tests/image_metrics_restate.py repeats the rule and the summation order in numpy.
 *
 * Inputs: a, b float [N][H][W][C], channel last (the layout of ls2fm_render_image's rgb), 1 <= C <= 4; mask uint8 [N][H][W] or
 * NULL, non-zero = counted; taps double [n_taps] ON THE HOST, n odd, 1 <= n <= LS2FM_IMAGE_MAX_TAPS, used along both axes (the
 * library evaluates no exp: a Gaussian and a uniform window are two tap arrays); c1, c2 doubles, >= 0 and finite.
 * THE RULE, every operation one rounded fp64 operation, none contracted, x = (double) a, y = (double) b:
 *   squared error  per pixel and channel (x - y)^2, over the pixels with mask != 0.  Per view: sse, and count = the number of
 *     pixel-channels (int64).
 *   SSIM  no padding: window (y, x), 0 <= y <= H - n, 0 <= x <= W - n, covers pixels (y .. y + n - 1, x .. x + n - 1); its centre
 *     pixel is (y + r, x + r), r = (n - 1) / 2.  Per channel the five moments E[x], E[y], E[xx], E[yy], E[xy] are the images
 *     x, y, x x, y y, x y blurred separably, along rows first:  R(y', x) = sum_k w[k] v(y', x + k),  then along columns:
 *     M(y, x) = sum_k w[k] R(y + k, x);  each sum is  acc = w[0] v[0];  acc = acc + w[k] v[k]  for k = 1 .. n - 1 in tap order.
 *     vx = E[xx] - mx mx,  vy = E[yy] - my my,  cxy = E[xy] - mx my,
 *     ssim = (((2 mx) my + c1) (2 cxy + c2)) / (((mx mx + my my) + c1) ((vx + vy) + c2)),  one IEEE division.
 *     Two identical images give exactly 1.0 at every window: numerator and denominator are the same operations.  Per view:
 *     ssim_sum over the windows whose centre pixel has mask != 0, all channels, and ssim_count = their number times C (int64).
 *   ssim_map  double [N][H - n + 1][W - n + 1][C] or NULL: every window's value, masked or not.
 * SUMMATION ORDER (no floating-point atomic, nothing read back): the image is cut into tiles of T x T, T = LS2FM_IMAGE_TILE,
 *   ceil(H / T) x ceil(W / T) of them; tile (ty, tx) owns the pixels (T ty + ly, T tx + lx) and the windows of the same indices,
 *   0 <= ly, lx < T.  Lane T ly + lx of the tile's workgroup starts from 0.0 and adds its pixel's (its window's) terms in channel
 *   order; a term that is not counted (outside the image, mask 0) is +0.0.  The T T = 256 lanes are added in the order of the
 *   library's workgroup sum (csrc/wave_ops.h block_sum: the xor butterfly 32, 16, .. 1 inside each wave of 64 lanes, then the
 *   four waves in index order).  A second launch adds a view's tiles in row-major tile order, starting from 0.0.  Neither the
 *   tile size nor a pixel's place in its tile shows in ssim_map; the sums depend on T through this order alone.
 * Views are independent: a non-finite pixel reaches the numbers of its own view only.  A view whose mask is empty gets sums
 * and counts of 0.  Two launches per call (one more per 65535 views), no allocation, no stream forked: the call can be captured.
 * workspace: ls2fm_image_compare_workspace_bytes(...) bytes (one partial row and two counts per view and tile); workspace_bytes
 * is what the caller provides.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL required array (mask and ssim_map are optional),
 * n_views < 1, channels outside 1 .. 4, n_taps even or outside 1 .. 33, height or width below n_taps, c1 or c2 negative or not
 * finite, H W C >= 2^31; LS2FM_ERR_WORKSPACE for a NULL or short workspace.  The size query refuses the same shapes with the
 * (negative) status as its result.
 */
#define LS2FM_IMAGE_TILE 16
#define LS2FM_IMAGE_MAX_TAPS 33
int64_t ls2fm_image_compare_workspace_bytes(int32_t n_views, int32_t height, int32_t width, int32_t channels, int32_t n_taps);
int ls2fm_image_compare(const float* a, const float* b, const uint8_t* mask, int32_t n_views, int32_t height, int32_t width,
                        int32_t channels, const double* taps, int32_t n_taps, double c1, double c2, double* sse, int64_t* count,
                        double* ssim_sum, int64_t* ssim_count, double* ssim_map, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * The radiance field at free points (csrc/radiance_points.hip behind ls2fm.mesh_colors.field_colors; an addition, the library
 * stays ABI 13): the colour the trained field gives a mesh vertex.  The reference evaluates radiance along camera rays only.
 *
 * Inputs: points float [n][3] (world); view_dirs float [n][3] or NULL; field, sdf_grid, rad_grid and params as ls2fm_render_fwd
 * takes them (rad_grid and the geo_* / rad_table parameters are read only with field->dual_field; n_samples and bgcolor are not
 * read).  Per point p, what Renderer.forward_composed forms per sample (models/Renderer.py:105-117):
 *   sdf, feats = SDF.infer_sdf(p, "ret_all");  g = SDF.gradient(p), the analytic normal, not normalised;
 *   view = Embedder_Fourier(v), v = view_dirs[i], or v = -g / max(|g|, 1e-12) when view_dirs is NULL (the surface seen head-on:
 *   -torch.nn.functional.normalize(g));  geo = feats[1:], with dual_field followed by Geometry_feat(p)[1:];
 *   rgb = infer_app([p, g, view, geo]).
 * Outputs: rgb float [n][3]; normal float [n][3] or NULL (g); sdf float [n] or NULL.  sdf and normal are bit for bit what
 * ls2fm_sdf_eval returns for the same points: the kernel runs that call's evaluators (sdf_point.h, render_common.h).
 * One lane per point, LS2FM_RADIANCE_POINTS_TILE points per workgroup; two launches (the weight preparation, the evaluation);
 * no atomic, no allocation, nothing read back, no stream forked: the call can be captured.  n = 0 returns at once.
 * workspace: ls2fm_radiance_points_workspace_bytes() bytes (the prepared weights).
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL descriptor, a grid descriptor the library does not
 * serve, a NULL required parameter or array, n < 0; LS2FM_ERR_UNSUPPORTED for field->bg_sdf (the composed form serves it);
 * LS2FM_ERR_WORKSPACE for a NULL workspace.
 */
#define LS2FM_RADIANCE_POINTS_TILE 256
int64_t ls2fm_radiance_points_workspace_bytes(void);
int ls2fm_radiance_points(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid, const ls2fm_grid_desc* rad_grid,
                          const ls2fm_params* params, const float* points, const float* view_dirs, int64_t n, float* rgb,
                          float* normal, float* sdf, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex colours of a mesh from photographs (csrc/mesh_colors.hip behind ls2fm.mesh_colors.photo_colors; additions, the library
 * stays ABI 13): per vertex, a weighted blend of the views that see it, visibility decided against ls2fm_rasterize's depth maps
 * of the same mesh.  The reference ships none.  tests/mesh_colors_restate.py repeats the rule in numpy.
 *
 * Inputs: verts float [V][3]; normals float [V][3] or NULL; poses float [N][3][4] and intr float [N][4] as for ls2fm_rasterize;
 * images float [N][H][W][C], channel last, 1 <= C <= 4; depth float [N][H][W], ls2fm_rasterize's depth of the same mesh, views
 * and near; masks uint8 [N][H][W] or NULL; near > 0; depth_tol >= 0; power, an integer 0 .. 8; and the caller-owned state
 * sums double [V][C + 1], count int32 [V] (zeroed by the caller before the first call).
 * THE VERTEX COLOUR RULE, per vertex and view, the views in index order:
 *   1. pixel     camera point c, projection (u, v), usable and IN THE IMAGE by the RASTERISATION RULE and ls2fm_mesh_mask_votes'
 *      rule above (csrc/raster_project.h holds the expressions for all three); the pixel is (floor u, floor v).  Otherwise the
 *      view is skipped.
 *   2. mask      a zero mask byte at the pixel skips the view.
 *   3. visible   d = depth at the pixel.  The view counts if and only if d is finite and c_z <= d + depth_tol * d, in fp32, the
 *      product and the sum each rounded once, not contracted.  An empty pixel (+inf) and a NaN fail.
 *   4. weight    without normals w = 1.  With normals, in fp64 from the fp32 inputs, every operation rounded once: n_c = R n,
 *      row r as ((R_r0 n_0 + R_r1 n_1) + R_r2 n_2);  dot = ((n_c0 c_0 + n_c1 c_1) + n_c2 c_2);  |n_c| = sqrt((n_c0 n_c0 +
 *      n_c1 n_c1) + n_c2 n_c2), |c| likewise, correctly rounded roots;  cos = (-dot) / (|n_c| |c|).  cos <= 0 or not finite
 *      skips the view.  w = 1, then w = w cos, `power` times.
 *   5. sample    bilinear about the pixel centres, in fp64: x = (double) u - 0.5, x0 = floor(x), fx = x - x0, y likewise; the
 *      columns x0, x0 + 1 and the rows y0, y0 + 1 clamped to the image; per channel r0 = a00 + fx (a10 - a00),
 *      r1 = a01 + fx (a11 - a01), s = r0 + fy (r1 - r0), a_xy the tap at column x, row y.
 *   6. accumulate  sums[v][c] += w s_c, sums[v][C] += w, count[v] += 1: the product rounded, then the sum.
 * One lane takes one vertex (LS2FM_MESH_COLORS_THREADS per workgroup) and loads, extends and stores its state: no atomic, and a
 * call over views 0 .. k followed by a call over views k + 1 .. N - 1 leaves the bits of one call over all of them.  A NaN pixel
 * stays in the sums of the vertices that sampled it.  One launch; n_verts = 0 and n_views = 0 return at once.
 * ls2fm_mesh_vertex_colors_finish  -> color float [V][C]: (float)(sums[v][c] / sums[v][C]) where count[v] > 0; elsewhere
 *   fallback[v][c] when fallback (float [V][C], on the device) is given, otherwise fill[c] (`channels` floats ON THE HOST, read
 *   before the call returns).  One launch.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL required array (normals, masks optional; one of
 * fallback and fill is required), a negative count, height or width outside [1, 32768], n_views height width >= 2^40, channels
 * outside 1 .. 4, power outside 0 .. 8, a near that is not positive and finite, a depth_tol that is negative or not finite.
 */
#define LS2FM_MESH_COLORS_THREADS 256
int ls2fm_mesh_vertex_colors(const float* verts, const float* normals, int64_t n_verts, const float* poses, const float* intr,
                             int32_t n_views, int32_t height, int32_t width, int32_t channels, const float* images,
                             const float* depth, const uint8_t* masks, float near, float depth_tol, int32_t power, double* sums,
                             int32_t* count, void* stream);
int ls2fm_mesh_vertex_colors_finish(const double* sums, const int32_t* count, int64_t n_verts, int32_t channels,
                                    const float* fallback, const float* fill, float* color, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TSDF fusion of posed depth maps into a dense volume (csrc/tsdf_fusion.hip behind ls2fm.fusion.integrate; an addition, the
 * library stays ABI 13): the way back from depth maps -- ls2fm_rasterize's, ls2fm_trace_image's, a sensor's -- to a surface.
 * The reference ships none.  tests/fusion_restate.py repeats the rule in numpy.
 *
 * The volume: nx x ny x nz lattice points, row-major with axis 2 fastest, as ls2fm_marching_cubes_* takes it.  Lattice point i
 * sits at X[a] = fl32(fl32((float) i[a] * voxel) + origin[a]): the vertex expression of ls2fm_marching_cubes_emit with
 * spacing = (voxel, voxel, voxel), so the mesh extracted from the volume is in the depth maps' world frame as it stands.
 * The caller owns the state tsdf float [nx][ny][nz] and weight float [nx][ny][nz], both zero for a fresh volume.
 * Inputs: depth float [N][H][W], camera z pixel for pixel (the convention of ls2fm_rasterize's depth); poses float [N][3][4] and
 * intr float [N][4] as for ls2fm_rasterize; view_weight float [N] or NULL (every view weighs 1); near, trunc, voxel > 0;
 * max_depth > 0 and max_weight > 0, either may be +inf; origin: 3 floats in HOST memory, read before the call returns.
 * THE FUSION RULE, per lattice point X and view v, the views in index order, every operation one rounded fp32 operation, none
 * contracted:
 *   1. pixel     camera point c, projection (u, v), usable and IN THE IMAGE by the RASTERISATION RULE and ls2fm_mesh_mask_votes'
 *      rule above (csrc/raster_project.h): the point lands on the pixel (floor u, floor v) on which the rasteriser would put a
 *      vertex at X.  Otherwise the view is skipped.
 *   2. depth     d = depth[v][py][px]: the nearest pixel, no interpolation.  Skipped unless d is finite, d > 0 and
 *      d <= max_depth: the rasteriser's empty pixels (+inf), a tracer's misses, a sensor's zeros and NaN all skip.
 *   3. weight    w = view_weight[v], or 1.  Skipped unless w > 0 (false for a NaN).
 *   4. distance  s = d - c_z: projective, along camera z, not along the ray.  Skipped if s < -trunc; s == -trunc counts.
 *   5. value     val = fminf(1, s / trunc).
 *   6. Wn = W + w;   7. T = ((W T) + (w val)) / Wn;   8. W = fminf(Wn, max_weight).
 * One lane takes one lattice point (a workgroup a brick of LS2FM_TSDF_BRICK_X x _Y x _Z points, consecutive lanes along axis
 * 2), loads its T and W once, walks the views and stores them once: no atomic, and a call over views 0 .. k followed by a call
 * over views k + 1 .. N - 1 leaves the bits of one call over all of them; a rerun and a graph replay repeat the bits.  One
 * launch, no workspace, no allocation, nothing read back, no stream forked: the call can be captured.  A volume with a side of
 * 0 and n_views = 0 return at once.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL required array (view_weight is optional), a negative
 * side or one above 2^24 (the index converts to fp32 exactly), 2^31 bricks or more, height or width outside [1, 32768],
 * n_views height width >= 2^40, near, trunc or voxel not positive and finite, max_depth or max_weight not positive (a NaN is
 * not), an origin that is not finite.
 */
#define LS2FM_TSDF_BRICK_X 2
#define LS2FM_TSDF_BRICK_Y 2
#define LS2FM_TSDF_BRICK_Z 64
int ls2fm_tsdf_integrate(float* tsdf, float* weight, int64_t nx, int64_t ny, int64_t nz, const float* origin, float voxel,
                         float trunc, const float* depth, const float* poses, const float* intr, const float* view_weight,
                         int32_t n_views, int32_t height, int32_t width, float near, float max_depth, float max_weight, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh simplification by vertex clustering with quadric error metrics (csrc/mesh_simplify.hip behind ls2fm.simplify; additions,
 * the library stays ABI 13): a mesh at marching-cubes density made small enough for a viewer, on the device.  Lindstrom's
 * out-of-core simplification (2000): one pass, order-free, a pure function of its inputs.  The reference ships none.
 * tests/simplify_restate.py repeats the rule in numpy.
 *
 * Inputs: verts float [V][3]; faces int32 [F][3], every index in [0, V) (the caller's duty: ls2fm.simplify checks it); cell, a
 * positive finite float; placement LS2FM_SIMPLIFY_QUADRIC or LS2FM_SIMPLIFY_MEAN; reg >= 0, finite (ls2fm.simplify: 2^-2);
 * colors float [V][C], 1 <= C <= 4, or NULL with C = 0.  THE CLUSTERING RULE.  All arithmetic is fp64 of the fp32 inputs, every
 * operation rounded once, none contracted.
 *   1. cell of a vertex   k_a = floor((double) v_a / (double) cell) per axis.  A vertex with a coordinate that is not finite is
 *      INVALID.  A finite vertex with a k_a outside [-2^20, 2^20) is BAD: it is counted (ls2fm.simplify raises ValueError from
 *      the count, the refusal of ls2fm.metrics.voxel_downsample) and otherwise treated as invalid.  key = x << 42 | y << 21 | z of
 *      the coordinates k_a + 2^20, as voxel_downsample packs them, so 0 <= key < 2^63; an invalid vertex has key -1.  The cell's centre is
 *      g_a = ((double) k_a + 0.5) * (double) cell: the sum is exact, the product rounds once.  The lattice is absolute: anchored
 *      at 0, not at the mesh's box.
 *   2. faces   a face is VALID iff its three vertices are valid (class 1), and SURVIVES iff it is valid and its three keys are
 *      pairwise distinct (class 2); class 0 otherwise.
 *   3. quadrics   corner k of a valid face CONTRIBUTES to its cell unless an earlier corner k' < k of the same face has the same
 *      key: a face adds its quadric once per distinct cell it touches.  For a contributing corner, with g its cell's centre and
 *      (a, b, c) the face's vertices in the face's order: p_i = (double) v_i - g;  u = p_b - p_a, w = p_c - p_a;
 *      n = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x), unnormalised (Lindstrom's area-squared weighting: no
 *      division, no square root);  d = (n_x p_a.x + n_y p_a.y) + n_z p_a.z.  The cell gains ten terms, sums 0 .. 9:
 *      n_x n_x, n_x n_y, n_x n_z, n_y n_y, n_y n_z, n_z n_z (A, upper triangle row-major), d n_x, d n_y, d n_z (b), d d.
 *   4. per-cell vertex sums   over the cell's valid vertices: the count m, p = (double) v - g per axis (sums 10 .. 12) and
 *      (double) colour per channel (sums 13 .. 12 + C).
 *   5. order of summation   the cell's vertices in ascending index and its contributing corners in ascending 3 f + k each form
 *      a SEGMENT, entries e_0, e_1, ...  One wave of 64 lanes sums a segment: lane l adds e_l, e_(l + 64), e_(l + 128), ... in
 *      that order into a running sum per quantity that starts at +0 (a lane without entries keeps +0); then the six
 *      butterfly steps o = 32, 16, 8, 4, 2, 1 replace every lane's sum s_l by s_l + s_(l xor o) (the library's wave_sum).  The
 *      result is lane 0's.  A segment of at most 64 entries is thus a balanced tree over its entries padded with +0 to 64.
 *   6. placement   mean_a = sum_p_a / (double) m.  t = (A00 + A11) + A22, lambda = reg * t;  (A + lambda I) x = b + lambda mean
 *      by the library's Cholesky solve (csrc/lm_math.h chol_solve at size 3: the matrix entries A_ij, the diagonal
 *      A_ii + lambda * 1, its g_i = -(b_i + lambda * mean_i); a pivot <= 0 or an x that is not finite fails).
 *      x = mean when placement is MEAN, when t is 0 or not finite, when the solve fails, or when any |x_a| > (double) cell / 2
 *      (false for no finite x_a).  The output vertex is (float) (g_a + x_a): one fp64 sum, one rounding to fp32, which may put
 *      it an ulp outside its cell.  The output colour is (float) (sum_c / (double) m).
 *   7. output   vertices: the cells that hold at least one corner of a surviving face, in ascending key order.  Faces: the
 *      surviving faces in input order, corner order kept, re-indexed to cell ranks; then every face that equals an earlier one
 *      as an oriented triangle (equal after rotating the smallest index to the front) is removed: the lowest input index stays
 *      (ls2fm.simplify does this with sorts of the triples; the library emits the faces it is told to keep).  vertex_map int32
 *      [V]: the output index of each input vertex's cell, -1 for an invalid vertex or a cell that is not output.
 * Stated, not fixed: clustering can create non-manifold edges and fold-overs; opposite-oriented duplicates both stay; no boundary
 * or feature-edge preservation beyond what the quadrics give; no texture coordinates; the absolute lattice (a translated mesh
 * simplifies differently).
 *
 * The calls, on one stream, with the caller's stable sorts and prefix sums between them; `workspace`
 * (ls2fm_mesh_simplify_workspace_bytes(V, F) bytes) carries state from mark to index to place and must not be touched between:
 *   keys   vert_key int64 [V], face_class uint8 [F] (may be NULL), counts int64 [2] = (surviving faces, bad vertices); counts
 *          is zeroed by the call.  With face_class NULL this is the whole of a face count.
 *   mark   sorted_key / sorted_vert int64 [V]: vert_key sorted ascending by a STABLE sort and the permutation.  Writes
 *          corner_head int32 [3F]: per corner 3 f + k the position in the sorted list of its cell's first vertex, 2^31 - 1 for a
 *          corner that does not contribute; head_used int32 [V]: 1 at the first sorted position of every output cell, else 0.
 *   index  head_rank int32 [V]: the inclusive prefix sum of head_used (its last entry is the number of output cells n_out).
 *          Writes vertex_map int32 [V] and face_index int32 [F][3]: a surviving face in output indices, (-1, -1, -1) otherwise.
 *   place  sorted_corner_head int32 [3F] / sorted_corner int64 [3F]: corner_head sorted ascending by a STABLE sort and the
 *          permutation.  stages: LS2FM_SIMPLIFY_STAGE_SUMS writes sums double [n_out][13 + C] and count int32 [n_out] (ONE WAVE
 *          per output cell), LS2FM_SIMPLIFY_STAGE_SOLVE reads them and writes out_verts float [n_out][3] and out_colors float
 *          [n_out][C]; both bits: both, in that order.
 *   emit   keep uint8 [F], keep_rank int32 [F] its inclusive prefix sum, n_kept its last entry: out_faces int32 [n_kept][3].
 * Nothing is read back by any call.  Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL array that is
 * needed, V < 0 or V >= 2^31, F < 0 or 3 F >= 2^31, a cell that is not positive and finite, C outside [0, 4] or C = 0 with colors
 * or C > 0 without, a placement or stages value not listed, a reg that is negative or not finite, n_out outside [0, V], n_kept
 * outside [0, F]; LS2FM_ERR_WORKSPACE for a NULL workspace or workspace_bytes below ls2fm_mesh_simplify_workspace_bytes(V, F).
 */
#define LS2FM_SIMPLIFY_SUMS 13
#define LS2FM_SIMPLIFY_QUADRIC 0
#define LS2FM_SIMPLIFY_MEAN 1
#define LS2FM_SIMPLIFY_STAGE_SUMS 1
#define LS2FM_SIMPLIFY_STAGE_SOLVE 2
int64_t ls2fm_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces);
int ls2fm_mesh_simplify_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float cell,
                             int64_t* vert_key, uint8_t* face_class, int64_t* counts, void* stream);
int ls2fm_mesh_simplify_mark(const int64_t* sorted_key, const int64_t* sorted_vert, int64_t n_verts, const int32_t* faces,
                             int64_t n_faces, const uint8_t* face_class, int32_t* corner_head, int32_t* head_used,
                             void* workspace, int64_t workspace_bytes, void* stream);
int ls2fm_mesh_simplify_index(const int32_t* head_used, const int32_t* head_rank, int64_t n_verts, const int32_t* faces,
                              int64_t n_faces, const uint8_t* face_class, int32_t* vertex_map, int32_t* face_index,
                              void* workspace, int64_t workspace_bytes, void* stream);
int ls2fm_mesh_simplify_place(const float* verts, const float* colors, int32_t channels, int64_t n_verts, const int32_t* faces,
                              int64_t n_faces, float cell, int32_t placement, double reg, const int64_t* sorted_key,
                              const int64_t* sorted_vert, const int32_t* sorted_corner_head, const int64_t* sorted_corner,
                              int64_t n_out, int32_t stages, double* sums, int32_t* count, float* out_verts, float* out_colors,
                              void* workspace, int64_t workspace_bytes, void* stream);
int ls2fm_mesh_simplify_emit(const int32_t* face_index, const uint8_t* keep, const int32_t* keep_rank, int64_t n_faces,
                             int64_t n_kept, int32_t* out_faces, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Plane-sweep multi-view stereo and the geometric-consistency filter of its depth maps (csrc/mvs_sweep.hip behind
 * ls2fm.mvs.plane_sweep and ls2fm.mvs.filter_depths; additions, the library stays ABI 13): from posed photographs to the depth
 * maps ls2fm_tsdf_integrate fuses, the classical dense baseline (COLMAP's patch_match_stereo and stereo_fusion) in its simplest
 * form.  The reference shells out to colmap for its sparse stage only and ships no dense stage.  tests/mvs_restate.py repeats
 * both rules in numpy, ls2fm.mvs.plane_sweep_torch and filter_depths_torch as torch ops; the three agree bit for bit.
 *
 * Conventions are the rasteriser's: poses world -> camera [3][4], intr float [V][4] = (fx, fy, cx, cy), pixel (px, py) has its
 * centre at u = px + 0.5, depth is camera z.  All views of a call share one image size H x W.
 * Inputs of the sweep: images float [V][H][W] (grey); refs int32 [R], the view index of each reference; sources int32 [R][S], an
 * entry outside [0, V) (-1 by convention) skips that source; depths float [R][D], the plane depths of each reference, formed by
 * the caller (the rule never forms them); rel float [R][S][3][4], P_rs = P_s o P_r^-1 formed in fp64 and rounded once by the
 * caller (entries of skipped sources are not read); half_width w in [1, LS2FM_MVS_MAX_HALF_WIDTH], n = (2 w + 1)^2 taps; near;
 * min_var >= 0; min_sources in [1, S].  A reference outside [0, V) has every pixel invalid.
 * THE SWEEP RULE, per reference r and pixel (px, py).  Every operation is one rounded fp32 operation, none contracted; division
 * and square root are correctly rounded; every sum starts at +0 and goes in the stated order.
 *   1. reference window   a pixel with px < w, px > W - 1 - w, py < w or py > H - 1 - w is INVALID.  Otherwise the taps a_i are
 *      the pixels (px + dx, py + dy), dy = -w .. w outer, dx = -w .. w inner (row-major).  ma = (sum a_i) / (float) n;
 *      va = sum (a_i - ma)^2.  The pixel is invalid if any tap is not finite or va < min_var (false for a NaN).  The
 *      mean-subtracted two-pass form is the rule: E[xx] - E[x]^2 cancels in fp32.
 *   2. warp   per tap pixel q = (qx, qy), plane k and source s: xn = (((float) qx + 0.5) - cx_r) / fx_r, yn likewise; the camera
 *      point of the reference is (xn d_k, yn d_k, d_k): the plane is fronto-parallel.  Its projection into s is the camera
 *      point / projection / usable part of the RASTERISATION RULE with the view (P_rs, intr_s) and `near`.
 *   3. sample   bilinear about pixel centres: x = u - 0.5, x0 = floor(x), tx = x - x0; y, y0, ty likewise.  The tap is valid
 *      iff usable and 0 <= x0, x0 <= W - 2, 0 <= y0, y0 <= H - 2 (fp32 comparisons; no clamping).  With b00, b10, b01, b11 the
 *      source pixels (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1): r0 = b00 + tx (b10 - b00), r1 = b01 + tx (b11 - b01),
 *      b = r0 + ty (r1 - r0).
 *   4. NCC   if any of the n taps is invalid or its b is not finite, (pixel, k, s) is invalid.  Otherwise mb and vb as in 1. and
 *      cov = sum (a_i - ma) (b_i - mb), all three in tap order.  Invalid if vb < min_var.  ncc = cov / sqrt(va vb).
 *   5. aggregate   score_k = (sum of ncc over the valid sources, in source order) / (float) count; invalid (NaN) if
 *      count < min_sources.
 *   6. select   the plane with the largest score; ties go to the lowest k; a NaN score never wins.  Without one the pixel is
 *      invalid.
 *   7. refine   with 0 < k < D - 1, s- = score_(k-1) and s+ = score_(k+1) both not NaN and den = (s- - 2 s0) + s+ < 0:
 *      off = (0.5 (s- - s+)) / den;  depth = d_k + off (d_(k+1) - d_k) for off >= 0, d_k + off (d_k - d_(k-1)) otherwise.  In
 *      every other case depth = d_k.
 * Outputs: depth float [R][H][W] (NaN where invalid), score float [R][H][W] (the winning score; NaN where invalid), plane int32
 * [R][H][W] (-1 where invalid).  One workgroup of 256 lanes per (reference, LS2FM_MVS_TILE x LS2FM_MVS_TILE tile); a pixel's
 * result depends on nothing but the rule, so references split over several calls leave the bits of one call.
 *
 * THE CONSISTENCY RULE (ls2fm_mvs_filter), one lane per (view r, pixel), same arithmetic.  Inputs: depth float [V][H][W];
 * sources int32 [V][S] (entries outside [0, V) skip); rel float [V][S][3][4] = P_rs and rel_back float [V][S][3][4] = P_sr, both
 * formed in fp64 and rounded once; max_reproj >= 0 (pixels), rel_depth >= 0, min_consistent >= 0.  For a pixel whose depth d is
 * finite and positive, and each source s in order:
 *   1. lift the pixel centre: uc = (float) px + 0.5, vc likewise; X = ((uc - cx_r) / fx_r) d, Y likewise; the point (X, Y, d)
 *   2. project it with the view (P_rs, intr_s) and `near`;  3. IN THE IMAGE by the rasteriser's floor rule gives the pixel
 *      (sx, sy), otherwise s is not consistent; d_s = depth[s][sy][sx]
 *   4. d_s finite and positive, otherwise not consistent
 *   5. lift (sx, sy)'s centre at d_s with intr_s as in 1.;  6. project it with the view (P_sr, intr_r): (u', v', z'), usable
 *   7. consistent iff du = u' - uc, dv = v' - vc, (du du) + (dv dv) <= max_reproj max_reproj, and |z' - d| <= rel_depth d.
 * Outputs: count uint8 [V][H][W], the number of consistent sources (0 for a pixel without a finite positive depth); filtered
 * float [V][H][W], the input depth where count >= min_consistent and NaN elsewhere.
 *
 * Both calls: one launch, no workspace, no atomics, nothing read back, no stream forked; they can be captured, and a rerun or a
 * replay repeats the bits.  n_refs = 0 (sweep) and n_views = 0 (filter) return at once.  Refused before anything is enqueued:
 * LS2FM_ERR_INVALID_ARGUMENT for a NULL array, height or width outside [1, 32768], views height width >= 2^40, S outside
 * [1, LS2FM_MVS_MAX_SOURCES], D outside [1, LS2FM_MVS_MAX_PLANES], a half width outside [1, LS2FM_MVS_MAX_HALF_WIDTH], near not
 * positive and finite, min_var, max_reproj or rel_depth negative or not finite, min_sources outside [1, S], a negative
 * min_consistent, 2^31 workgroups or more.
 */
#define LS2FM_MVS_TILE 16
#define LS2FM_MVS_MAX_HALF_WIDTH 5
#define LS2FM_MVS_MAX_SOURCES 64
#define LS2FM_MVS_MAX_PLANES 65536
int ls2fm_mvs_sweep(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs, int32_t n_refs,
                    const int32_t* sources, int32_t n_sources, const float* depths, int32_t n_planes, const float* rel,
                    const float* intr, int32_t half_width, float near, float min_var, int32_t min_sources, float* depth,
                    float* score, int32_t* plane, void* stream);
int ls2fm_mvs_filter(const float* depth, int32_t n_views, int32_t height, int32_t width, const int32_t* sources, int32_t n_sources,
                     const float* rel, const float* rel_back, const float* intr, float near, float max_reproj, float rel_depth,
                     int32_t min_consistent, uint8_t* count, float* filtered, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PatchMatch stereo with slanted planes (csrc/mvs_patchmatch.hip behind ls2fm.mvs.plane_score, patch_match_step and patch_match;
 * additions, the library stays ABI 13): per pixel of a reference a plane hypothesis (d, n) -- d the camera z at the pixel centre,
 * n its normal in the reference camera's frame, not necessarily of unit length -- scored by the sweep's NCC over a window warped
 * along that plane, and improved by red-black propagation and random refinement (COLMAP's patch_match_stereo, Gipuma, ACMH).  The
 * state is depth float [R][H][W], normal float [R][H][W][3], score float [R][H][W].  tests/patchmatch_restate.py repeats both rules
 * in numpy, ls2fm.mvs.plane_score_torch and patch_match_step_torch as torch ops; the three agree bit for bit.
 *
 * Conventions, images, refs, sources, rel = P_rs, intr, half_width w, near, min_var and min_sources are the sweep's, and so is the
 * arithmetic: every operation is one rounded fp32 operation, none contracted; division is correctly rounded; a square root is
 * taken in fp64 of the fp32 argument and rounded to fp32; every sum starts at +0 and goes in tap / source order.
 * The window has a tap step t in {1, 2}: dx and dy take the values -w, -w + t, ... <= w, dy outer and dx inner, n = (2 w / t + 1)^2
 * taps (integer division).  t = 1 is the sweep's window.
 *
 * THE PLANE SCORE of the hypothesis (d, n) at pixel p = (px, py) of reference r:
 *   0. reference window   step 1 of THE SWEEP RULE over the taps of the step t: ma, va, and the pixel INVALID as there.
 *   1. lift   xn_p = (((float) px + 0.5) - cx_r) / fx_r, yn_p likewise;  g_p = ((n_x xn_p) + (n_y yn_p)) + n_z.
 *   2. the hypothesis is INVALID unless d is finite and d > 0, n_x, n_y and n_z are finite, and g_p < 0 (the plane faces the
 *      camera; false for a NaN).
 *   3. h = g_p d.
 *   4. per tap q: xn_q, yn_q and g_q as in 1.; d_q = h / g_q.  The tap is invalid unless g_q < 0 and d_q is finite.
 *   5. the tap's camera point is (xn_q d_q, yn_q d_q, d_q).
 *   6. steps 2 (its projection with the view (P_rs, intr_s) and `near`), 3 (sample), 4 (NCC over the n taps) and 5 (aggregate) of
 *      THE SWEEP RULE follow unchanged: score, NaN when invalid or count < min_sources.
 * With n = (0, 0, -1) and t = 1, g = -1 and d_q = d exactly: the score at d_k is the sweep's score_k by its bits.
 *
 * THE DRAWS.  mix(x), on 32-bit unsigned integers that wrap:  x ^= x >> 16;  x *= LS2FM_MVS_MIX_A;  x ^= x >> 15;
 * x *= LS2FM_MVS_MIX_B;  x ^= x >> 15.  key = mix(mix(mix(mix(seed + LS2FM_MVS_MIX_SALT) + view) + iteration) + (py W + px)), with
 * `view` the VIEW index refs[r], so that chunks of references do not show in the bits;  u_j = (float) (mix(key + j) >> 8) 2^-24,
 * exact, in [0, 1), j = 0 .. 8.  normalise(x, y, z): s = ((x x) + (y y)) + (z z), root = sqrt(s), (x / root, y / root, z / root).
 *
 * THE PATCHMATCH STEP (colour, iteration) updates, in place, the pixels with (px + py) & 1 == colour that have a window (step 1 of
 * THE SWEEP RULE's bounds).  The incumbent is the pixel's stored (d, n, score); its score is not evaluated again.  A candidate
 * replaces the incumbent iff its PLANE SCORE is not NaN and either the incumbent's score is NaN or the candidate's is strictly
 * larger.  The candidates, in this order:
 *   1. the eight neighbours m = p + (0,-1), (-1,0), (1,0), (0,1), (0,-3), (-3,0), (3,0), (0,3) (dx, dy): all at odd Manhattan
 *      distance, so every pixel read has the other colour and the step is free of races in place and independent of the order the
 *      lanes run in.  A neighbour outside the image, or whose depth is not finite and positive, is skipped.  With g_m formed from
 *      m's normal at m's own lift, and g = ((n_mx xn_p) + (n_my yn_p)) + n_mz at p's: the candidate ((g_m d_m) / g, n_m).
 *   2. perturbed depth   (d (1 + rho_d ((2 u_0) - 1)), n), about the incumbent at that moment (as are 3. and 4.)
 *   3. perturbed normal  (d, normalise(n_x + rho_n ((2 u_1) - 1), n_y + rho_n ((2 u_2) - 1), n_z))
 *   4. both              the depth of 2. with u_3, the normal of 3. with u_4 and u_5
 *   5. a fresh hypothesis   d = 1 / (i0 + u_6 (i1 - i0)), i0 = 1 / d_min[r], i1 = 1 / d_max[r];
 *      n = normalise(sigma ((2 u_7) - 1), sigma ((2 u_8) - 1), -1)
 * 2. to 4. are skipped while the incumbent's score is NaN (there is no hypothesis to perturb).  rho_d, rho_n (already scaled by
 * the caller's schedule rho 2^-iteration, formed in fp64 and rounded once), sigma = max_slope, d_min and d_max float [R] arrive
 * as fp32.  A reference outside [0, V) is left as it is by the step and gets NaN scores from ls2fm_mvs_plane_score.
 *
 * ls2fm_mvs_plane_score writes THE PLANE SCORE of a given state at every pixel (NaN for a pixel without a window);
 * ls2fm_mvs_patchmatch_step is one half-sweep of one colour.  One workgroup of 256 lanes per (reference, tile of
 * LS2FM_MVS_PM_TILE_H x LS2FM_MVS_PM_TILE_W pixels), one lane per pixel of a colour.  Both calls: one launch, no workspace, no
 * atomics, nothing read back, no stream forked; they can be captured, and a rerun of the same state repeats the bits.  n_refs = 0
 * returns at once.  Refused before anything is enqueued (LS2FM_ERR_INVALID_ARGUMENT): what ls2fm_mvs_sweep refuses, a tap step
 * outside {1, 2}, a colour outside {0, 1}, a negative iteration, rho_d, rho_n or sigma negative or not finite.
 */
#define LS2FM_MVS_PM_TILE_H 16
#define LS2FM_MVS_PM_TILE_W 32
#define LS2FM_MVS_PM_DRAWS 9
#define LS2FM_MVS_MIX_A 0x21F0AAADu
#define LS2FM_MVS_MIX_B 0x735A2D97u
#define LS2FM_MVS_MIX_SALT 0x9E3779B9u
int ls2fm_mvs_plane_score(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs, int32_t n_refs,
                          const int32_t* sources, int32_t n_sources, const float* rel, const float* intr, int32_t half_width,
                          int32_t tap_step, float near, float min_var, int32_t min_sources, const float* depth, const float* normal,
                          float* score, void* stream);
int ls2fm_mvs_patchmatch_step(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs,
                              int32_t n_refs, const int32_t* sources, int32_t n_sources, const float* rel, const float* intr,
                              int32_t half_width, int32_t tap_step, float near, float min_var, int32_t min_sources, int32_t colour,
                              int32_t iteration, uint32_t seed, float rho_d, float rho_n, float sigma, const float* d_min,
                              const float* d_max, float* depth, float* normal, float* score, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fusion of per-view depth and normal maps into one oriented, coloured cloud (csrc/mvs_fuse.hip behind ls2fm.mvs.fuse_depths;
 * additions, the library stays ABI 13): COLMAP's stereo_fusion, the stage between patch_match_stereo and poisson_mesher.
 * tests/fuse_restate.py repeats the rule in numpy, ls2fm.mvs.fuse_depths_torch as torch ops; the three agree bit for bit.
 *
 * Conventions are those of THE CONSISTENCY RULE.  Inputs: depth float [V][H][W], meant to be ls2fm_mvs_filter's output (any value
 * that is not finite and positive is "no depth"); normal float [V][H][W][3] in each camera's frame, of any length, or NULL; colour
 * float [V][H][W][C], C in [1, 4], or NULL with C = 0; sources int32 [V][S], rel = P_rs, rel_back = P_sr, intr, near, max_reproj
 * and rel_depth exactly as ls2fm_mvs_filter takes them; cos2 in [0, 1], the squared cosine of the largest angle between the normals
 * of a pixel and a partner, formed by the caller; cam_to_world float [V][3][4] = P_v^-1, formed in fp64 and rounded once by the
 * caller; a range of views [view_begin, view_end).
 * THE FUSION RULE, per view r of the range and pixel (px, py) whose depth d is finite and positive:
 *   1. partners   each source s in order; an entry outside [0, V) and an entry equal to r are skipped, a view listed twice counts
 *      twice.  Steps 1 to 7 of THE CONSISTENCY RULE, unchanged, give the partner pixel (sx, sy) of view s with its depth d_s, and
 *      whether it is consistent.  With normals it must pass one more test: with n_r the pixel's normal, n_s the partner pixel's and
 *      B = P_sr, n'_i = ((B_i0 n_sx) + (B_i1 n_sy)) + B_i2 n_sz;  a = ((n_rx n'_x) + (n_ry n'_y)) + n_rz n'_z;  rr = ((n_rx n_rx) +
 *      (n_ry n_ry)) + n_rz n_rz, ss likewise of n'; consistent only if a > 0 and a a >= cos2 (rr ss).  Every operation is one
 *      rounded fp32 operation, none contracted; every comparison is false for a NaN.
 *   2. ownership   the pixel gives a point iff no consistent partner has a view index below r.  support = 1 + the number of
 *      consistent partners for a pixel that gives a point and 0 for every other pixel.  The maps are filtered already, so a consistent
 *      partner pixel is one that itself survived: a surface element seen by several views is emitted by the lowest of them and the
 *      others are folded into its mean -- no visited mask, no atomics, no dependence on an order.
 *   3. the point   the mean over the contributors: the pixel itself, then its consistent partners in source order.  A contributor's
 *      camera point (X, Y, d) is that of its own pixel centre, the fp32 values of step 1 (the pixel) or 5 (a partner) of THE
 *      CONSISTENCY RULE.  With M = cam_to_world of the contributor's own view, in fp64 of the fp32 values and never contracted:
 *      w_i = ((M_i0 X + M_i1 Y) + M_i2 d) + M_i3.  The sums start at +0; point_i = (float) (sum_i / (double) support).
 *      The normal: per contributor g_i = (M_i0 n_x + M_i1 n_y) + M_i2 n_z in fp64, l = sqrt((g_0 g_0 + g_1 g_1) + g_2 g_2), the
 *      unit vector g_i / l; their sum t in the same order; normal_i = (float) (t_i / sqrt((t_0 t_0 + t_1 t_1) + t_2 t_2)).  A zero
 *      or NaN sum gives a NaN normal in its own row and nothing else.  Division and root are correctly rounded.  A normal that faces
 *      its camera keeps facing it: M's rotation is R^T, as in ls2fm.mvs.normals_to_world.
 *      The colour: per channel the fp64 sum of the contributors' own pixels, divided by (double) support and rounded once.
 * Outputs: support uint8 [V][H][W], written for the views of the range only; rows in (view, py, px) order: points float [M][3],
 * normals float [M][3] (with normals), colours float [M][C] (with colours), pixel int64 [M] = (v H + py) W + px of the owner.
 * Deviations from COLMAP's stereo_fusion, on purpose: a mean, not a median; partners come from the source lists alone, there is no
 * traversal beyond one hop; the nearest pixel, not an interpolated one; no min_num_pixels inside the rule, the caller thresholds
 * support; near-duplicates remain where consistency is not mutual.
 *
 * ls2fm_mvs_fuse_mark writes support.  The caller forms row int64 [view_end - view_begin][H][W], the exclusive prefix sum of
 * support > 0 over the pixels of the range in (view, py, px) order plus the number of rows of the views before the range, and
 * ls2fm_mvs_fuse_emit repeats the walk of every pixel with support > 0 and writes its row; a row outside [0, n_rows) is not
 * written.  Both: one launch, one lane per pixel, a workgroup of 256 lanes takes one tile of LS2FM_MVS_FUSE_TILE_W x
 * LS2FM_MVS_FUSE_TILE_H pixels of one view (a wave is two rows of 32 pixels), no workspace, no atomics, nothing read back, no stream forked; they can be captured, a rerun or a replay repeats the bits, and the view ranges of several
 * calls leave the bits of one.  n_views = 0, an empty range and (emit) n_rows = 0 return at once.  Refused before anything is
 * enqueued (LS2FM_ERR_INVALID_ARGUMENT): what ls2fm_mvs_filter refuses of the arguments they share, a NULL array, normals without
 * normal (emit) or the reverse, colours without colour or the reverse, C outside [1, 4] with colour or not 0 without, a view range
 * outside [0, V] or with its end before its begin, cos2 outside [0, 1] or not finite, a negative n_rows, 2^31 workgroups or more.
 */
#define LS2FM_MVS_FUSE_MAX_CHANNELS 4
#define LS2FM_MVS_FUSE_TILE_W 32
#define LS2FM_MVS_FUSE_TILE_H 8
int ls2fm_mvs_fuse_mark(const float* depth, const float* normal, int32_t n_views, int32_t height, int32_t width,
                        const int32_t* sources, int32_t n_sources, const float* rel, const float* rel_back, const float* intr,
                        float near, float max_reproj, float rel_depth, float cos2, int32_t view_begin, int32_t view_end,
                        uint8_t* support, void* stream);
int ls2fm_mvs_fuse_emit(const float* depth, const float* normal, const float* colour, int32_t n_channels, int32_t n_views,
                        int32_t height, int32_t width, const int32_t* sources, int32_t n_sources, const float* rel,
                        const float* rel_back, const float* intr, const float* cam_to_world, float near, float max_reproj,
                        float rel_depth, float cos2, int32_t view_begin, int32_t view_end, const uint8_t* support,
                        const int64_t* row, int64_t n_rows, float* points, float* normals, float* colours, int64_t* pixel,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * Texture atlases of a mesh (csrc/mesh_texture.hip behind ls2fm.texture; additions, the library stays ABI 13): the map from
 * texels to surface points, where ls2fm_mesh_vertex_colors and ls2fm_radiance_points put colour, and the render of a textured
 * mesh from ls2fm_rasterize's face ids and barycentrics.  The reference ships none.  tests/texture_restate.py repeats both
 * rules in numpy.
 *
 * THE ATLAS RULE.  The atlas is a square of S x S texels, S a power of two in [4, 32768]; texel (x, y) has its centre at
 * (x + 0.5, y + 0.5).  Every face gets a right-isosceles chart; two charts share one square cell of pitch p = 2^k texels.  With the
 * gutter g >= 0 the admissible classes are the k with 2 g + 4 <= 2^k <= the largest pitch (256 by default), and L = p - 2 g - 3.
 *   corners   a face's corners are its vertices; a face with an index outside [0, V) has NaN corners.
 *   rotation  e_i = the squared length of the edge opposite corner i: the fp32 differences of the two other corners, component by
 *     component, converted to fp64, then ((dx dx + dy dy) + dz dz) in fp64.  r = 0; r = 1 if e_1 > e_0; r = 2 if e_2 > max so far:
 *     the corner opposite the longest edge, ties to the lowest index, a NaN never greater.  The chart's corners a, b, c are the
 *     face's corners r, r + 1, r + 2 (mod 3): the orientation is kept, a sits on the right angle.
 *   class     l2 = the larger of the two e_i other than e_r (the legs at a).  The class is the smallest admissible k with
 *     l2 <= T_k, T_k = ((2^k - 2 g - 3) texel)^2 formed on the host in doubles (the product, then its square); the largest
 *     admissible k if there is none (the face is undersampled); the smallest if a corner is not finite.  Only fp64 sums, products
 *     and comparisons: torch ops on the device and numpy give the same classes.
 *   packing   order[slot] = face: the faces sorted stably by class, descending.  Slots 2 c and 2 c + 1 of a class's slots share
 *     cell c of that class.  A cell's Morton offset is the sum of p^2 over all earlier cells (sizes are powers of four in
 *     descending order, so the sum is a multiple of the cell's own p^2); the cell's origin (x0, y0) is that offset de-interleaved,
 *     bit 2 b of the offset to bit b of x0, bit 2 b + 1 to bit b of y0.  The atlas holds the mesh iff the cells' total area is at
 *     most S^2.
 *   in a cell  with i = x - x0, j = y - y0: the texel belongs to chart A (the even slot) iff i + j <= p - 1, otherwise to chart B
 *     (the odd slot), which is A turned by 180 degrees about the cell's centre: i' = p - 1 - i, j' = p - 1 - j (for A i' = i,
 *     j' = j).  A's corners a, b, c sit on the centres of the texels (i', j') = (g, g), (g + L, g), (g, g + L).  A texel of a cell
 *     behind the last, of chart B of an odd last slot, or whose order entry lies outside [0, F) is unowned.
 *     For every point of the closed chart triangle every bilinear tap of non-zero weight is a texel owned by that face
 *     (tests/test_texture_host.py proves it for every admissible p <= 64 and g <= 3): colour never bleeds between charts.
 *   surface   fp32, every operation rounded once, none contracted: s = (float)(i' - g) / (float) L, t likewise from j'; per
 *     component X = (a + s (b - a)) + t (c - a); gutter texels extrapolate (s or t negative, or s + t > 1).  The normal is
 *     n = (b - a) x (c - a), n_x = d1_y d2_z - d1_z d2_y and cyclically with d1 = b - a, d2 = c - a, not normalised.  Unowned
 *     texels get face = -1 and NaN point and normal; so does, for point and normal, an owned texel of a face with an index
 *     outside [0, V).
 * ls2fm_texture_texels  the rows [row_begin, row_end) of the atlas -> face int32 [rows][S], point float [rows][S][3], normal
 *   float [rows][S][3], and uv float [F][3][2] (or NULL): the texel that sits on a chart corner writes that corner's texel
 *   coordinates (its own centre: half-integers) at the face's own corner index (r + q) mod 3; the other entries are not
 *   touched.  Inputs: verts, faces as for ls2fm_rasterize; order int32 [F]; rot int32 [F] (taken into [0, 2]);
 *   class_log2_pitch int32 [n_classes] and class_count int64 [n_classes] ON THE HOST, read before the call returns: the classes'
 *   k, strictly descending, and how many faces each holds (0 allowed).  One lane per texel in LS2FM_TEXTURE_TILE-square tiles
 *   aligned to the atlas; the lane forms its Morton code, finds its class against the at most LS2FM_TEXTURE_MAX_CLASSES class
 *   starts (kernel arguments), its cell by a shift, its slot by the half of the cell.  One launch, no atomic, no workspace,
 *   nothing read back: the call can be captured; bands leave the bits of one call.  row_begin = row_end returns at once.
 *
 * THE TEXTURE RENDER RULE, per pixel with face f = face_id and barycentrics (w0, w1, w2), exactly as ls2fm_rasterize writes them:
 *   f < 0 or f >= F gives the background.  Otherwise, in fp32, every operation rounded once, none contracted, with (x_i, y_i) =
 *   uv[f][i]:  x = ((w0 x0 + w1 x1) + w2 x2), y likewise.  The sample is step 3 of THE SWEEP RULE about the texel centres with
 *   clamped taps in place of the validity test: sx = x - 0.5, u0 = floor(sx), tx = sx - u0; u0 is taken into [-1, S] as a float
 *   (a NaN becomes -1) and converted; the columns u0, u0 + 1 and the rows likewise are clamped to [0, S - 1]; per channel
 *   r0 = b00 + tx (b10 - b00), r1 = b01 + tx (b11 - b01), out = r0 + ty (r1 - r0).  A NaN texel stays in the pixels that tap it.
 * ls2fm_texture_render  face_id int32 [N][H][W], bary float [N][H][W][3], uv float [F][3][2], texture float [S][S][C], 1 <= C <= 4,
 *   background float [C] ON THE HOST (read before the call returns) -> out float [N][H][W][C].  One lane per pixel, one launch,
 *   no atomic: the call can be captured.  n_views = 0 returns at once.
 * Refused before anything is enqueued: LS2FM_ERR_INVALID_ARGUMENT for a NULL required array (uv of ls2fm_texture_texels is
 * optional; verts, faces, order, rot and uv are required only when there are vertices / faces), a negative count, n_faces >= 2^31,
 * S that is not a power of two in [4, 32768], a band that is not 0 <= row_begin <= row_end <= S, channels outside 1 .. 4, height
 * or width outside [1, 32768], n_views height width >= 2^40, a gutter outside [0, 64], n_classes outside
 * [1, LS2FM_TEXTURE_MAX_CLASSES], a class table that is not strictly descending, holds a k outside [2, 15] or with
 * 2^k < 2 g + 4, whose counts do not add up to n_faces, or whose cells do not fit S^2.
 */
#define LS2FM_TEXTURE_TILE 16
#define LS2FM_TEXTURE_MAX_CLASSES 8
int ls2fm_texture_texels(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* order,
                         const int32_t* rot, int32_t n_classes, const int32_t* class_log2_pitch, const int64_t* class_count,
                         int32_t gutter, int32_t size, int32_t row_begin, int32_t row_end, int32_t* face, float* point,
                         float* normal, float* uv, void* stream);
int ls2fm_texture_render(const int32_t* face_id, const float* bary, int32_t n_views, int32_t height, int32_t width, const float* uv,
                         int64_t n_faces, const float* texture, int32_t size, int32_t channels, const float* background, float* out,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lens-distortion camera models and image undistortion (csrc/camera_model.h, csrc/undistort.hip behind ls2fm.undistort; additions,
 * the library stays ABI 13): COLMAP's image_undistorter, the stage between mapper and patch_match_stereo.  Every other stage knows
 * the pinhole camera intr = (fx, fy, cx, cy) alone; these two calls are the adapter in front of them.  tests/undistort_restate.py
 * repeats both rules in numpy, ls2fm.undistort._undistort_images_torch and _camera_points_torch as torch ops; the three agree bit
 * for bit.
 *
 * A camera is LS2FM_CAMERA_PARAMS = 12 numbers (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6): OpenCV's rational model, COLMAP's
 * FULL_OPENCV.  SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL and OPENCV are the same rule with zeros.
 * THE DISTORTION RULE, from an undistorted normalised point (x, y) to the distorted image, in the precision T of the call (fp32 or
 * fp64), every operation rounded once, none contracted, division correctly rounded:
 *   r2  = (x x) + (y y)
 *   num = 1 + r2 (k1 + r2 (k2 + r2 k3))            Horner, innermost first
 *   den = 1 + r2 (k4 + r2 (k5 + r2 k6))
 *   rad = num / den
 *   xy  = x y
 *   xd  = (x rad) + ( ((2 p1) xy) + (p2 (r2 + (2 x) x)) )
 *   yd  = (y rad) + ( (p1 (r2 + (2 y) y)) + ((2 p2) xy) )
 *   u   = (fx xd) + cx ;  v = (fy yd) + cy
 * Its Jacobian J = d(xd, yd)/d(x, y) = [a b; c d], analytic, in the same precision and with the same r2, den and rad:
 *   dnum = k1 + r2 ((2 k2) + r2 (3 k3)) ;  dden = k4 + r2 ((2 k5) + r2 (3 k6))
 *   g   = (dnum - (rad dden)) / den               d rad / d r2
 *   gx  = (2 x) g ;  gy = (2 y) g
 *   a   = ((rad + (x gx)) + ((2 p1) y)) + (p2 (6 x))
 *   b   = ((x gy) + ((2 p1) x)) + (p2 (2 y))
 *   c   = ((y gx) + (p1 (2 x))) + ((2 p2) y)
 *   d   = ((rad + (y gy)) + (p1 (6 y))) + ((2 p2) x)
 * Deviations from COLMAP, on purpose: no fisheye, FOV or thin-prism models (atan is not a correctly rounded operation and the rule
 * would lose its bits); no guard against a rational model that folds over (rad not monotone in r): such a camera maps several
 * undistorted points to one photograph pixel and the rule takes it at its word.
 *
 * ls2fm_undistort_images  images float [V][Hs][Ws][C], channel last, 1 <= C <= 4, the photographs; cam float [V][12] their cameras;
 *   out_intr float [V][4] the pinhole cameras of the outputs; the output size H x W, which need not be the source's; mode
 *   LS2FM_UNDISTORT_BILINEAR or LS2FM_UNDISTORT_NEAREST; fill float [C] ON THE HOST, read before the call returns (NaN is the useful
 *   value: ls2fm_mvs_sweep and PatchMatch treat a non-finite tap as invalid) -> out float [V][H][W][C] and valid uint8 [V][H][W] (or
 *   NULL).  THE UNDISTORTION RULE, per view and output pixel (px, py), fp32, every operation rounded once, none contracted:
 *   1. xn = (((float) px + 0.5) - cx_o) / fx_o, yn = (((float) py + 0.5) - cy_o) / fy_o with (fx_o, fy_o, cx_o, cy_o) = out_intr.
 *   2. (u, v) by THE DISTORTION RULE with the view's cam.
 *   3. the pixel is valid iff u and v are finite and IN THE IMAGE of the source by the rasteriser's comparisons, 0 <= u < Ws and
 *      0 <= v < Hs in fp32.  Otherwise it takes fill and valid = 0.  A NaN or infinite camera word, or den == 0, makes u or v
 *      non-finite (or NaN) and the pixel takes fill.
 *   4. bilinear: x = u - 0.5, x0 = floor(x), tx = x - x0, rows likewise from v; the columns x0, x0 + 1 and the rows y0, y0 + 1
 *      are clamped to the image as in step 5 of THE VERTEX COLOUR RULE; per channel r0 = a00 + tx (a10 - a00),
 *      r1 = a01 + tx (a11 - a01), out = r0 + ty (r1 - r0), a_xy the tap at column x, row y.  A NaN source pixel stays in the pixels
 *      that tap it (also with weight 0).
 *   5. nearest: the source pixel (floor u, floor v), copied.  For depth maps and masks: a blend of depths across an edge invents
 *      surfaces.
 *   One lane per output pixel; a workgroup of 256 lanes takes one tile of LS2FM_UNDISTORT_TILE_W x LS2FM_UNDISTORT_TILE_H output
 *   pixels of one view, so the view's 16 camera words are scalar loads.  One launch, no workspace, no atomics, nothing read back:
 *   the call can be captured, a rerun or a replay repeats the bits, and the views of several calls leave the bits of one.
 *   n_views = 0 returns at once.
 *
 * ls2fm_camera_points  key points, both directions, fp64, every operation rounded once, none contracted.  uv double [N][2];
 *   view_start int32 [V + 1], non-decreasing, 0 <= view_start[0], view_start[V] <= N: the points of view v are the rows
 *   view_start[v] .. view_start[v + 1] - 1 (the convention of ls2fm_absolute_pose); cam double [V][12]; out_intr double [V][4];
 *   iters in [0, LS2FM_CAMERA_MAX_ITERS] -> uv_out double [N][2] and residual double [N] (or NULL).  A row outside
 *   [view_start[0], view_start[V]) is not written.  One lane per point finds its view by bisection of view_start (the last v
 *   with view_start[v] <= row): a table that is not monotone makes no access outside the arrays, only rows of unspecified views.
 *   direction = LS2FM_CAMERA_DISTORT:  (x, y) = ((u - cx_o) / fx_o, (v - cy_o) / fy_o), the pinhole out_intr undone; uv_out = THE
 *     DISTORTION RULE's (u, v) with cam; residual = 0.
 *   direction = LS2FM_CAMERA_UNDISTORT:  xd = (u - cx) / fx, yd = (v - cy) / fy with cam's own words; start at (x, y) = (xd, yd);
 *     exactly `iters` Newton steps: (fx_, fy_) = the rule's (xd, yd) at (x, y) with its Jacobian, e_x = fx_ - xd, e_y = fy_ - yd,
 *     det = (a d) - (b c), x = x - (((d e_x) - (b e_y)) / det), y = y - (((a e_y) - (c e_x)) / det).  A step whose det is zero or
 *     not finite is skipped, along with all later ones; the trip count is `iters` for every lane, nothing is read back.
 *     uv_out = ((fx_o x) + cx_o, (fy_o y) + cy_o);  residual = ((fx e_x)(fx e_x)) + ((fy e_y)(fy e_y)) with e of the final iterate:
 *     the squared pixel distance in the photograph, for the caller to drop what did not converge.
 *   One launch of LS2FM_CAMERA_POINTS_THREADS lanes per workgroup, no workspace, no atomics: capturable; chunks of rows with the
 *   same tables, a rerun and a replay leave the same bits.  n_points = 0 returns at once.
 * Refused before anything is enqueued (LS2FM_ERR_INVALID_ARGUMENT): a NULL required array (valid and residual are optional), a
 * negative count, a height or width of the source or the output outside [1, 32768], V Hs Ws or V H W >= 2^40, C outside 1 .. 4, an
 * unknown mode or direction, iters outside [0, LS2FM_CAMERA_MAX_ITERS], n_points >= 2^31, n_views < 1 with points, 2^31 workgroups
 * or more.
 */
#define LS2FM_CAMERA_PARAMS 12
#define LS2FM_CAMERA_MAX_ITERS 32
#define LS2FM_CAMERA_DISTORT 0
#define LS2FM_CAMERA_UNDISTORT 1
#define LS2FM_CAMERA_POINTS_THREADS 256
#define LS2FM_UNDISTORT_BILINEAR 0
#define LS2FM_UNDISTORT_NEAREST 1
#define LS2FM_UNDISTORT_TILE_W 32
#define LS2FM_UNDISTORT_TILE_H 8
int ls2fm_undistort_images(const float* images, int32_t n_views, int32_t src_height, int32_t src_width, int32_t channels,
                           const float* cam, const float* out_intr, int32_t height, int32_t width, int32_t mode, const float* fill,
                           float* out, uint8_t* valid, void* stream);
int ls2fm_camera_points(const double* uv, int64_t n_points, const int32_t* view_start, int32_t n_views, const double* cam,
                        const double* out_intr, int32_t direction, int32_t iters, double* uv_out, double* residual, void* stream);

/* ---------------------------------------------------------------------------------------------
 * How the table-gradient scatter (inside ls2fm_render_bwd / ls2fm_sdf_points_bwd) finishes the few coarse levels whose slabs
 * are split over several workgroups.  Process-wide; takes effect for the calls enqueued afterwards.
 *   1 (default; env LS2FM_SCATTER_MODE)  every part's 64-bit fixed-point partial sums are combined by one more small launch:
 *      integer sums, so every table-gradient entry is the exactly rounded sum of its fp32 contributions whatever the order
 *      the hardware produced them in, and a backward repeats itself bit for bit
 *   0  the parts flush with float atomics into a zeroed range: one launch fewer, sums of rounded partials in arrival order
 *      (what rounds 1-3 shipped; kept for measurements)
 * tcnn's kernel_grid_backward is atomicAdd on fp32/half2 throughout (non-deterministic); the reference has no switch.
 */
int ls2fm_set_scatter_mode(int mode);
int ls2fm_get_scatter_mode(void);

/* ---------------------------------------------------------------------------------------------
 * Opt-in per-kernel timing (benchmarking aid; the library's only process-global state, off by default).
 * While enabled, every internal kernel launch of the calls above is bracketed by HIP events recorded on the
 * call's own stream; ls2fm_profile_get() synchronises those events and returns, per internal kernel, the
 * accumulated device time in milliseconds and the number of launches.  While enabled, the calls launch their kernels
 * serially on `stream` (the internal side-stream overlap is off) so that each span is the kernel's own duration.
 * Single-threaded use.
 */
int ls2fm_profile_enable(int on);
int ls2fm_profile_reset(void);
int ls2fm_profile_count(void);
const char* ls2fm_profile_name(int index);
int ls2fm_profile_get(int index, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* LS2FM_H */
