// cvo_track_kernels.hip -- the device step between the two align launches of a K-stream tracker step (include/cvo_hip.h: cvo_tracks_*).
//
// The tracker aligns a frame twice (local_tracker.cpp:356, 415): cvo_odometry against the previous frame, then cvo_keyframe against the
// keyframe, warm-started from the odometry result by reset_initial (cvo.cpp:611-618, local_tracker.cpp:407).  cvo_tracks_step_async queues
// both launches at once; this kernel sits between them on the stream and turns the odometry launch's device-resident results into the
// keyframe launch's device-resident start states, so the host does not have to wait for the first launch before it can queue the second.
// One lane per stream; the arithmetic is cvo_math.hpp's reset_initial_eval, the very functions the host's cvo_reset_initial calls.
#include <hip/hip_runtime.h>
#include "cvo_device.h"
#include "cvo_math.hpp"

namespace cvohip {

// keyframe start state of stream i: R, T from reset_initial(odometry transform) -- or as carried when the odometry alignment did not return
// CVO_OK (that keyframe alignment's result is dropped by the host) --, ell, transform and iter as carried, everything else zero
__global__ void cvo_track_link_kernel(const TrackLinkIn* __restrict__ in, const PairState* __restrict__ odo_states, PairState* __restrict__ key_states,
                                      TrackLinkOut* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TrackLinkIn q = in[i];
    const PairState* so = odo_states + q.odo_state;
    const int status = so->status;
    float R[9], T[3], inv[12];
    if (status == 0) {
        float od[12];
        for (int k = 0; k < 12; ++k) od[k] = so->transform[k];
        reset_initial_eval(q.transform, od, R, T, inv);
    } else {
        for (int k = 0; k < 9; ++k) R[k] = q.R[k];
        for (int k = 0; k < 3; ++k) T[k] = q.T[k];
        for (int k = 0; k < 12; ++k) inv[k] = 0.f;
    }
    PairState* sk = key_states + q.key_state;
    unsigned* w = reinterpret_cast<unsigned*>(sk);
    for (unsigned k = 0; k < sizeof(PairState) / sizeof(unsigned); ++k) w[k] = 0u;
    for (int k = 0; k < 9; ++k) sk->R[k] = R[k];
    for (int k = 0; k < 3; ++k) sk->T[k] = T[k];
    sk->ell = q.ell;
    for (int k = 0; k < 12; ++k) sk->transform[k] = q.transform[k];
    sk->iter = q.iter;
    TrackLinkOut o;
    for (int k = 0; k < 9; ++k) o.R[k] = R[k];
    for (int k = 0; k < 3; ++k) o.T[k] = T[k];
    for (int k = 0; k < 12; ++k) o.init_inverse[k] = inv[k];
    o.odo_status = status; o.pad_[0] = o.pad_[1] = o.pad_[2] = 0;
    out[i] = o;
}

// cvo_selftest_reset_initial: reset_initial_eval on caller inputs, n x {transform[12], odometry[12]} -> n x {R[9], T[3], init_inverse[12]}
__global__ void selftest_reset_initial_kernel(const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float tr[12], od[12], R[9], T[3], inv[12];
    for (int k = 0; k < 12; ++k) { tr[k] = in[(size_t)i * 24 + k]; od[k] = in[(size_t)i * 24 + 12 + k]; }
    reset_initial_eval(tr, od, R, T, inv);
    for (int k = 0; k < 9; ++k) out[(size_t)i * 24 + k] = R[k];
    for (int k = 0; k < 3; ++k) out[(size_t)i * 24 + 9 + k] = T[k];
    for (int k = 0; k < 12; ++k) out[(size_t)i * 24 + 12 + k] = inv[k];
}

hipError_t launch_track_link(const TrackLinkIn* in, const PairState* odo_states, PairState* key_states, TrackLinkOut* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(cvo_track_link_kernel, dim3((n + 63) / 64), dim3(64), 0, s, in, odo_states, key_states, out, n);
    return hipGetLastError();
}
hipError_t launch_selftest_reset_initial(const float* in, float* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(selftest_reset_initial_kernel, dim3((n + 63) / 64), dim3(64), 0, s, in, out, n);
    return hipGetLastError();
}

}  // namespace cvohip
