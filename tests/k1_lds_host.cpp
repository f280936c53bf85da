// Host build of k1_lds.h for tests/test_abi.py (g++): the LDS K1 asks for, as launch_gauss and make_geom compute it.
#include "../linesegmentdetector-slam_amd/csrc/k1_lds.h"
extern "C" {
long k1_lds_bytes(double sca, int tapR, int* IWp, int* IHmax) {
    const lsdhip::K1Lds r = lsdhip::k1_lds(sca, tapR);
    if (IWp) *IWp = r.IWp;
    if (IHmax) *IHmax = r.IHmax;
    return (long)r.bytes;
}
int k1_tile_w(void) { return lsdhip::kK1TileW; }
int k1_tile_h(void) { return lsdhip::kK1TileH; }
}
