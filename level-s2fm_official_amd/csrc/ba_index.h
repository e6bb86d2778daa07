// The observation index of the two bundle adjustments (bundle_adjust.hip: Adam; bundle_adjust_lm.hip: Levenberg-Marquardt), built
// once per loop by their prepare calls.  Every array the kernels index through is the library's OWN validated copy in the
// workspace (view_start, obs_point, the point -> observations CSR), so a caller's index can never take a kernel out of bounds
// after prepare has accepted it.  A workspace counts as prepared only while its header [8] = {magic, V, P, n, 0 ...} stands:
// prepare clears it first and writes it last.
#pragma once

#include <vector>

#include "ls2fm_device.h"

namespace ba_index {

inline bool sizes_ok(int64_t V, int64_t P, int64_t n) { return V >= 1 && V <= (1 << 20) && P >= 1 && P <= (1 << 28) && n >= 1 && n <= (1 << 28); }

struct Index {
    std::vector<int32_t> view_start;   // [V + 1]
    std::vector<int32_t> obs_point;    // [n]
    std::vector<int32_t> obs_view;     // [n]: the position of the observation's view
    std::vector<int32_t> point_start;  // [P + 1]
    std::vector<int32_t> point_obs;    // [n]: observations of point p in list order (= rising view position)
};

// not prepared until the header is written again, at the end
inline bool clear_header(int32_t* header, hipStream_t stream) {
    static const int32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyAsync(header, none, sizeof(none), hipMemcpyHostToDevice, stream) == hipSuccess;
}

// h -> d on the stream; h must outlive the caller's next synchronisation
template <typename T>
inline bool upload(T* d, const std::vector<T>& h, hipStream_t stream) {
    return hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream) == hipSuccess;
}

// The index arrays are read back ONCE, here (loop construction, outside any iteration; one synchronisation, which also completes
// whatever the caller enqueued before), checked, and the point -> observations CSR is built by a stable counting sort.
// LS2FM_ERR_LAUNCH for a failed copy, LS2FM_ERR_INVALID_ARGUMENT for content.
inline int build(const int32_t* view_start, const int32_t* obs_point, int64_t V, int64_t P, int64_t n, hipStream_t stream, Index* ix) {
    std::vector<int32_t>&vs = ix->view_start, &op = ix->obs_point, &ov = ix->obs_view, &ps = ix->point_start, &po = ix->point_obs;
    vs.resize(V + 1); op.resize(n); ov.resize(n); ps.assign(P + 1, 0); po.resize(n);
    if (hipMemcpyAsync(vs.data(), view_start, 4 * (V + 1), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(op.data(), obs_point, 4 * n, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    LS2FM_CHECK_ARG(vs[0] == 0 && vs[V] == n);
    for (int64_t v = 0; v < V; ++v) LS2FM_CHECK_ARG(vs[v + 1] > vs[v]);            // sorted by view, and no view without an observation
    for (int64_t i = 0; i < n; ++i) LS2FM_CHECK_ARG(op[i] >= 0 && op[i] < P);
    for (int64_t v = 0; v < V; ++v)
        for (int64_t i = vs[v]; i < vs[v + 1]; ++i) ov[i] = (int32_t)v;
    for (int64_t i = 0; i < n; ++i) ++ps[op[i] + 1];
    for (int64_t p = 0; p < P; ++p) ps[p + 1] += ps[p];
    std::vector<int32_t> cur(ps.begin(), ps.end() - 1);
    for (int64_t i = 0; i < n; ++i) po[cur[op[i]]++] = (int32_t)i;
    return LS2FM_OK;
}

}  // namespace ba_index
