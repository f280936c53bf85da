// fa_relocate_host.h -- the host side of the relocalisation entries (lsd_enqueue_fa_lost_gather_device, lsd_enqueue_fa_carry_seed_device
// and their host conveniences; include/lsd_hip.h) that needs no device: the argument checks and the element counts of the staging
// regions.  Plain C++, no HIP: lsd_loc.hip uses it, and tests/fa_relocate_host.cpp drives it under the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/lsd_hip.h"

namespace lsdhip {

inline bool fa_misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// What the host conveniences hand the checks below in the place of a HOST pointer: null stays null, anything else becomes an aligned
// address -- the device entries' alignment rules are about device memory, which the conveniences' own staging supplies.
inline const void* fa_host_stand_in(const void* p) {
    alignas(16) static const char aligned = 0;
    return p ? &aligned : nullptr;
}

// lsd_enqueue_fa_lost_gather_device's refusals; scan_cap is the context's scan capacity (has_ctx false: a null context)
inline bool fa_lost_refused(bool has_ctx, int scan_cap, const void* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch,
                            const void* scans, const void* lens, int stride, const void* key, int max_lost, const void* scans_out,
                            const void* lens_out, const void* pick, const void* n_lost) {
    return !has_ctx || !carry || !poses || !scans || !lens || !scans_out || !lens_out || !pick || !n_lost || n_seq < 1 || n_seq > 65536 ||
           frames_pitch < 1 || frames_pitch > 4096 || pose_pitch < 24 || pose_pitch % 8 != 0 || stride < 1 || stride > scan_cap || max_lost < 1 ||
           max_lost > 4096 || fa_misaligned(carry, 8) || fa_misaligned(poses, 8) || fa_misaligned(scans, 16) || fa_misaligned(scans_out, 16) ||
           fa_misaligned(key, 4) || fa_misaligned(lens, 4) || fa_misaligned(lens_out, 4) || fa_misaligned(pick, 4) || fa_misaligned(n_lost, 4);
}

// lsd_enqueue_fa_carry_seed_device's refusals
inline bool fa_seed_refused(bool has_ctx, const void* carry, int n_seq, int frames_pitch, const void* pick, int n_pick, const void* loc,
                            const void* resp, const lsd_fa_seed_par& par, const void* rep) {
    auto bad = [](double v) { return !std::isfinite(v) || v < 0; };
    return !has_ctx || !carry || !pick || !loc || n_seq <= 0 || frames_pitch < 1 || frames_pitch > 4096 || n_pick < 1 || n_pick > 4096 ||
           par.max_best == 0 || bad(par.var_xy) || bad(par.var_ang) || bad(par.cov_scale) || bad(par.floor_xy) || bad(par.floor_ang) ||
           (!resp && (!(par.var_xy > 0) || !(par.var_ang > 0))) || fa_misaligned(carry, 8) || fa_misaligned(loc, 8) || fa_misaligned(resp, 8) ||
           fa_misaligned(rep, 8) || fa_misaligned(pick, 4);
}

// The element counts of lsd_fa_lost_gather's staging regions, in size_t: n_seq * frames_pitch * stride reaches 2^40 readings.
struct FaLostStage { size_t carries, slots, readings, rows, readings_out; };
inline FaLostStage fa_lost_stage(int n_seq, int frames_pitch, int stride, int max_lost) {
    const size_t slots = (size_t)n_seq * (size_t)frames_pitch;
    return {(size_t)n_seq, slots, slots * (size_t)stride, (size_t)max_lost, (size_t)max_lost * (size_t)stride};
}

// a length outside 0..stride (the host convenience's own refusal); -1: none
inline long long fa_lost_bad_len(const int* lens, size_t slots, int stride) {
    for (size_t i = 0; i < slots; i++)
        if (lens[i] < 0 || lens[i] > stride) return (long long)i;
    return -1;
}

}  // namespace lsdhip
