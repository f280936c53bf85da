#!/usr/bin/env python3
"""Pack the replay logs of the reference into tests/golden/ (run in the build container only):
  localize_data.npz   data/: odometry + map parameters (its lidar frames are tests/golden/lidar.npz, its map "mapValue" of maps.npz)
  localize_f3key.npz  data_20190513/data_f3key/data1: lidar frames, odometry, map parameters (map: "f3key" of maps.npz)
  localize_f4key.npz  data_20190514/data_f4key/data1: the same (map: "f4key")

The fixture is DATA, read with the driver's own conventions (LSD/main_on_windows.cpp:27-61):
  * mapParam.txt: oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY;
  * Lidar.txt: 360 "range angle" readings per frame ("inf": no return; the loop drops those, :115-121);
  * Odom.txt: one "x y ang" row per replayed frame; the driver's feof loop appends ONE MORE row after the last line, because the
    file ends in a newline and the loop tests feof before the fscanf that fails.  That row is uninitialised in the reference
    (a stack structPosition); it is ASSUMED here to repeat the last row (what fscanf leaves in a reused stack slot), so that the
    last frame sees a zero odometry step.  Nobody can run the reference here to confirm it.  Then Odom[0].x = 0.
The stored vector has the quirks applied ("odom", frames + 1 rows) and the raw rows ("odom_raw").  The loop stops after frame
Odom.size() - 1 (:183), i.e. after as many frames as Odom.txt has rows: the f3key / f4key logs hold one lidar frame more than that,
which the driver never replays (stored all the same, "n_frames" says how many are replayed).
"""
import os
import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def odom_vector(path):
    raw = np.loadtxt(path).reshape(-1, 3)
    assert open(path).read().endswith("\n")
    odom = np.concatenate([raw, raw[-1:]], 0)          # the feof loop's extra row (assumed to repeat the last one, see above)
    odom[0, 0] = 0.0                                   # Odom[0].x = 0 (:61)
    return raw, odom


def map_param(d):
    p = open(os.path.join(d, "mapParam.txt")).read().split()
    return np.array([float(v) for v in p[:5]], np.float64)


LOGS = {  # name: (directory, lidar frames in the file, frames replayed)
    "f3key": ("data_20190513/data_f3key/data1", 280, 279),
    "f4key": ("data_20190514/data_f4key/data1", 274, 273),
}


def main():
    d = os.path.join(REF, "data")
    raw, odom = odom_vector(os.path.join(d, "Odom.txt"))
    lid = np.load(os.path.join(HERE, "lidar.npz"))["lidar"]
    assert raw.shape == (99, 3) and lid.shape[0] == 99 and odom.shape == (100, 3), (raw.shape, lid.shape)
    out = os.path.join(HERE, "localize_data.npz")
    np.savez_compressed(out, odom=odom, odom_raw=raw, map_param=map_param(d), n_frames=np.int32(99))
    print("wrote", out, os.path.getsize(out), "bytes")
    for name, (sub, n_lidar, n_rep) in LOGS.items():
        d = os.path.join(REF, sub)
        raw, odom = odom_vector(os.path.join(d, "Odom.txt"))
        lid = np.loadtxt(os.path.join(d, "Lidar.txt")).reshape(-1, 360, 2)
        assert lid.shape[0] == n_lidar and raw.shape == (n_rep, 3) and odom.shape == (n_rep + 1, 3), (name, lid.shape, raw.shape)
        out = os.path.join(HERE, "localize_%s.npz" % name)
        np.savez_compressed(out, lidar=lid.astype(np.float64), odom=odom, odom_raw=raw, map_param=map_param(d), n_frames=np.int32(n_rep))
        assert os.path.getsize(out) < 1 << 20
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
