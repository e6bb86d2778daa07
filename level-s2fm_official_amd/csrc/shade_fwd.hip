// shade_fwd: the training forward's shading kernel (the chain is described in shade_fwd.h, the body is shade_fwd_body.inc).
#include "shade_fwd.h"

namespace {

// CT = 16-column tiles (of consecutive samples) per wave: 4 -> a wave covers 64 samples with ~250 registers (2 waves/SIMD);
// 2 -> 32 samples per wave, half the per-lane state, twice the waves (4 per SIMD) to hide the chain's latencies behind.
// FULL (round 6, as in shade_bwd.hip): all 32 encoding channels of both grids live AND the ray's samples fill every wave's tiles (N a
// multiple of 16 CT: every lane's samples live, aligned for the vector form) -- known at compile time: no per-channel predicates, no
// scalar-load fallback paths, the operand loads are straight-line code.
template <bool DUAL, int MAXS, int CT, bool FULL = false>
__global__ void __launch_bounds__(MAXS * 4 / CT, CT == 2 ? 4 : 2)
shade_fwd_kernel(FieldC fc, int ch1_arg, int ch2_arg, const Packed* __restrict__ pk, const float* __restrict__ center,
                 const float* __restrict__ ray, int64_t p_pad, const float* __restrict__ E1,
                 const float* __restrict__ J1, const float* __restrict__ E2, float* __restrict__ rgb_out,
                 float* __restrict__ sdfs_out, float* __restrict__ normals_out, float* __restrict__ depth_out,
                 float* __restrict__ nm_out, float* __restrict__ SDFV, float* __restrict__ NRM,
                 float* __restrict__ RGBS, float* __restrict__ FE, float* __restrict__ FE2, float* __restrict__ ROUT,
                 float* __restrict__ LPART, int64_t r_pad, ls2fm_loss_spec loss) {
    constexpr bool SAVE = true;
    float* const op_out = nullptr;
#include "shade_fwd_body.inc"
}

}  // namespace

int ls2fm_launch_shade_fwd(const FieldC& fc, int dual, int ch1, int ch2, const Packed* pk, const float* center, const float* ray,
                           int64_t n_rays, const WsLayout& w, float* ws, float* rgb, float* sdfs_volume, float* normals,
                           float* depth_mlp, float* normal_mlp, const ls2fm_loss_spec* loss, hipStream_t s) {
    // up to 256 samples per ray: two tiles per wave (4 waves/SIMD; 71.6 -> 66.1 us at the benchmark); longer rays keep four
    // (a 1024-thread workgroup of the two-tile form does not fit the register budget of 4 waves/SIMD without spilling into LDS)
    const bool small = fc.n_samples <= 256;
    const int per_wave = small ? 32 : 64;
    const int threads = (fc.n_samples + per_wave - 1) / per_wave * 64;
    ls2fm_loss_spec ls{};            // rgb_gt == null: plain render
    if (loss) ls = *loss;
    const bool full = small && ch1 == 32 && (!dual || ch2 == 32) && fc.n_samples % 32 == 0;
#define LS2FM_SHADE_FWD(DUAL, MAXS, CT, FULL)                                                                      \
    shade_fwd_kernel<DUAL, MAXS, CT, FULL><<<(unsigned)n_rays, threads, 0, s>>>(                                    \
        fc, ch1, ch2, pk, center, ray, w.p_pad, ws + w.e1, ws + w.j1, DUAL ? ws + w.e2 : nullptr, rgb, sdfs_volume, \
        normals, depth_mlp, normal_mlp, ws + w.sdfv, ws + w.nrm, ws + w.rgbs, ws + w.fe, DUAL ? ws + w.fe2 : nullptr,        \
        ws + w.rout, ws + w.lpart, w.r_pad, ls)
    if (dual) { if (full) LS2FM_SHADE_FWD(true, 256, 2, true); else if (small) LS2FM_SHADE_FWD(true, 256, 2, false); else LS2FM_SHADE_FWD(true, 512, 4, false); }
    else      { if (full) LS2FM_SHADE_FWD(false, 256, 2, true); else if (small) LS2FM_SHADE_FWD(false, 256, 2, false); else LS2FM_SHADE_FWD(false, 512, 4, false); }
#undef LS2FM_SHADE_FWD
    return LS2FM_OK;
}
