// k_rdp_lds.h -- the LDS a workgroup of the long FeatureScan kernel (k_rdp_long.hip) needs, as a function of the launch's stride alone.
//
// Shared by the launch (which sizes its dynamic LDS by it) and lsd_set_scan_capacity (which refuses a capacity whose scans would not
// fit the device's LDS before anything is enqueued), as k1_lds.h is for K1.  Plain C++, no HIP.
#pragma once
#include <stddef.h>

namespace lsdhip {

constexpr int kRdpShortMaxLen = 1024;               // strides up to here run on k_rdp (static LDS); the default scan capacity
constexpr int kRdpLongMaxLen = 4096;                // LSD_SCAN_MAX_LEN: the long kernel's 15-bit indices would hold 32767

// Per reading of the stride: px, py (2 x fp64); cs, ce and the two halves of the span stack / break list / chord-point list
// (4 x u16); brk / mark and split (2 x u8).  26 bytes: 27.4 KiB at 1081 readings, 104 KiB at 4096.
inline size_t rdp_long_lds(int stride) {
    const size_t s = (size_t)stride;
    return (s * (2 * sizeof(double) + 4 * sizeof(unsigned short) + 2) + 15) & ~(size_t)15;
}

}  // namespace lsdhip
