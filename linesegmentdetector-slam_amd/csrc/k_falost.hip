// k_falost.hip -- the lost robots of a tick picked and their scans packed into a batch of a fixed size (lsd_enqueue_fa_lost_gather_device;
// include/lsd_hip.h; restated in tests/fa_relocate_cases.py): what lsd_enqueue_grid_locate_device is given when only the
// robots without a pose are to be located.  One launch, no workspace, no atomics: the ranks are a prefix count in ascending s.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsd_internal.h"

namespace lsdhip {

// Workgroup b of G = min(max_lost, kFaLostGroups) owns the ranks j with j % G == b.  Every workgroup makes the same pass over the
// sequences, kFaLostThreads at a time in ascending s -- a lane decides "lost" for its sequence and searches its slot; a ballot and mbcnt
// give its rank inside the wavefront, four LDS words the wavefronts in front of it, a running base the chunks in front of those -- and keeps
// the picks of its own ranks in LDS.  Behind the pass it copies the rows of its ranks, 16 bytes per lane and step.  The pass is repeated
// by every workgroup (G times n_seq carries' first words and keys; the slot search only for sequences without a pose): the price of one
// launch without a second kernel or a counter in memory, small against the copy and the search that follows.
constexpr int kFaLostThreads = 256, kFaLostGroups = 128, kFaLostMaxLost = 4096;
constexpr int kFaLostOwn = kFaLostMaxLost / kFaLostGroups;          // ranks per workgroup at the largest max_lost
static_assert(sizeof(lsd_polar) == 16, "a reading is one 16-byte access");

__global__ __launch_bounds__(kFaLostThreads) void k_fa_lost_gather(const lsd_fa_carry* __restrict__ carry, int n_seq, int frames_pitch,
                                                                   const unsigned char* __restrict__ poses, size_t pose_pitch,
                                                                   const lsd_polar* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                                   const int32_t* __restrict__ key_of, int32_t key, int max_lost,
                                                                   lsd_polar* __restrict__ scans_out, int* __restrict__ lens_out,
                                                                   int32_t* __restrict__ pick, int32_t* __restrict__ n_lost) {
    __shared__ int s_w[kFaLostThreads / 64];
    __shared__ int s_pick[kFaLostOwn];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, G = (int)gridDim.x, b = (int)blockIdx.x;
    int base = 0;                                                  // the lost sequences in front of this chunk
    for (int s0 = 0; s0 < n_seq; s0 += kFaLostThreads) {
        const int s = s0 + tid;
        int slot = -1;
        if (s < n_seq && (!key_of || key_of[s] == key)) {
            const double* x = carry[s].state.x;
            const double x0 = x[0];
            if (fabs(x0 + 1) < 0.0001) {                           // the "no pose" test of the re-base and the correction (a NaN is not lost)
                const long long k0 = __double_as_longlong(x0), k1 = __double_as_longlong(x[1]), k2 = __double_as_longlong(x[2]);
                const size_t first = (size_t)s * (size_t)frames_pitch;
                for (int t = frames_pitch - 1; t >= 0; t--) {      // the LARGEST t: bytes, not values, and the frame had a scan
                    const long long* p = reinterpret_cast<const long long*>(poses + (first + (size_t)t) * pose_pitch);
                    if (p[0] == k0 && p[1] == k1 && p[2] == k2 && lens[first + (size_t)t] > 0) { slot = t; break; }
                }
            }
        }
        const bool lost = slot >= 0;
        const unsigned long long m = __ballot(lost);
        const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kFaLostThreads / 64; k++) {
            const int v = s_w[k];
            if (k < w) off += v;
            total += v;
        }
        const int j = base + off + before;
        if (lost && j < max_lost && j % G == b) s_pick[j / G] = s * frames_pitch + slot;
        base += total;
        __syncthreads();                                           // s_w is rewritten by the next chunk; s_pick is read behind the loop
    }
    const int n_got = min(base, max_lost);
    if (b == 0 && tid == 0) { n_lost[0] = base; n_lost[1] = n_got; }
    for (int j = b; j < max_lost; j += G) {
        if (j >= n_got) {                                          // a row past the gathered ones: an empty scan; its readings keep their bytes
            if (tid == 0) { lens_out[j] = 0; pick[j] = -1; }
            continue;
        }
        const int from = s_pick[j / G];
        const lsd_polar* src = scans + (size_t)from * (size_t)stride;
        lsd_polar* dst = scans_out + (size_t)j * (size_t)stride;
        for (int i = tid; i < stride; i += kFaLostThreads) dst[i] = src[i];
        if (tid == 0) { lens_out[j] = lens[from]; pick[j] = from; }
    }
}

void launch_fa_lost_gather(const lsd_fa_carry* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch, const lsd_polar* scans,
                           const int* lens, int stride, const int32_t* key_of, int32_t key, int max_lost, lsd_polar* scans_out, int* lens_out,
                           int32_t* pick, int32_t* n_lost, hipStream_t st) {
    const int groups = max_lost < kFaLostGroups ? max_lost : kFaLostGroups;
    hipLaunchKernelGGL(k_fa_lost_gather, dim3(groups), dim3(kFaLostThreads), 0, st, carry, n_seq, frames_pitch,
                       static_cast<const unsigned char*>(poses), pose_pitch, scans, lens, stride, key_of, key, max_lost, scans_out, lens_out, pick,
                       n_lost);
}

}  // namespace lsdhip
