#!/usr/bin/env python3
"""Pack the replay logs of the reference into tests/golden/, and survey all of them (run in the build container only):
  localize_data.npz       data/: odometry + map parameters (its lidar frames are tests/golden/lidar.npz, its map "mapValue" of maps.npz)
  localize_f3key.npz      data_20190513/data_f3key/data1: lidar frames, odometry, map parameters, way-points (map: "f3key" of maps.npz)
  localize_f4key.npz      data_20190514/data_f4key/data1: the same (map: "f4key")
  localize_f3key_<N>.npz  data_20190513/data_f3key/data<N>, localize_f4key_<N>.npz: data_20190514/data_f4key/data<N> (all logs of a
                          key share one map and one mapParam.txt)
  localize_survey.json    `survey`: all 19 recorded logs replayed on the CPU (the oracle's FeatureScan and matching with glibc's libm,
                          then tests/fa_restatement.py), one record per log (tests/fa_logs.py: summary)

    make_localize_logs.py                    the three fixtures of LOGS
    make_localize_logs.py pack f3key_9 ...   the named logs
    make_localize_logs.py survey             localize_survey.json, and the selection that follows from it

The fixture is DATA, read with the driver's own conventions (LSD/main_on_windows.cpp:27-61):
  * mapParam.txt: oriMapCol, oriMapRow, mapResol, mapOriX, mapOriY;
  * Lidar.txt: 360 "range angle" readings per frame ("inf": no return; the loop drops those, :115-121);
  * Odom.txt: one "x y ang" row per replayed frame; the driver's feof loop appends ONE MORE row after the last line, because the
    file ends in a newline and the loop tests feof before the fscanf that fails.  That row is uninitialised in the reference
    (a stack structPosition); it is ASSUMED here to repeat the last row (what fscanf leaves in a reused stack slot), so that the
    last frame sees a zero odometry step.  Nobody can run the reference here to confirm it.  Then Odom[0].x = 0.
  * realPos.txt: surveyed way-points "x y" in metres; recored_Odom.txt: the frame count (1-based, tests/fa_logs.py) at which the
    robot stood on each.  Stored as "real_pos" [k, 2] and "recorded" [k].
The stored vector has the quirks applied ("odom", frames + 1 rows) and the raw rows ("odom_raw").  The loop stops after frame
Odom.size() - 1 (:183), i.e. after as many frames as Odom.txt has rows: the logs hold one lidar frame more than that (data6 of f4key:
none), which the driver never replays (stored all the same, "n_frames" says how many are replayed).  Where every frame of a log has
the same angle column, the frames are stored as "lidar_range" [n, 360] and "lidar_angle" [360] (fa_restatement.log_lidar), otherwise
whole as "lidar" [n, 360, 2].
"""
import json
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = {"f3key": ("data_20190513/data_f3key", 9), "f4key": ("data_20190514/data_f4key", 10)}
SURVEY = os.path.join(HERE, "localize_survey.json")


def odom_vector(path):
    raw = np.loadtxt(path).reshape(-1, 3)
    assert open(path).read().endswith("\n")
    odom = np.concatenate([raw, raw[-1:]], 0)          # the feof loop's extra row (assumed to repeat the last one, see above)
    odom[0, 0] = 0.0                                   # Odom[0].x = 0 (:61)
    return raw, odom


def map_param(d):
    p = open(os.path.join(d, "mapParam.txt")).read().split()
    return np.array([float(v) for v in p[:5]], np.float64)


def log_dir(name):
    """f3key / f4key: data1 of the key (the first fixtures' names); f3key_<N>: data<N>."""
    key, _, num = name.partition("_")
    return os.path.join(REF, KEYS[key][0], "data%s" % (num or "1"))


def all_logs():
    return ["%s_%d" % (k, i) for k, (_, n) in KEYS.items() for i in range(1, n + 1)]


def read_log(name):
    d = log_dir(name)
    raw, odom = odom_vector(os.path.join(d, "Odom.txt"))
    lid = np.loadtxt(os.path.join(d, "Lidar.txt")).reshape(-1, 360, 2).astype(np.float64)
    n = len(raw)
    assert lid.shape[0] in (n, n + 1) and odom.shape == (n + 1, 3), (name, lid.shape, raw.shape)
    real = np.loadtxt(os.path.join(d, "realPos.txt")).reshape(-1, 2)
    rec = np.array(open(os.path.join(d, "recored_Odom.txt")).read().split(), np.int32)
    assert len(real) == len(rec) and (np.diff(rec) > 0).all() and 1 <= rec[0] and rec[-1] <= n, (name, rec)
    return dict(lidar=lid, odom=odom, odom_raw=raw, map_param=map_param(d), n_frames=np.int32(n), real_pos=real, recorded=rec)


def pack(name):
    log = read_log(name)
    lid = log.pop("lidar")
    if (lid[:, :, 1] == lid[0, :, 1]).all():           # one angle column for the whole log: store it once
        log.update(lidar_range=lid[:, :, 0], lidar_angle=lid[0, :, 1])
    else:
        log["lidar"] = lid
    out = os.path.join(HERE, "localize_%s.npz" % name)
    np.savez_compressed(out, **log)
    assert os.path.getsize(out) < 1 << 20
    print("wrote", out, os.path.getsize(out), "bytes,", int(log["n_frames"]), "frames replayed")


def pack_data():
    d = os.path.join(REF, "data")
    raw, odom = odom_vector(os.path.join(d, "Odom.txt"))
    lid = np.load(os.path.join(HERE, "lidar.npz"))["lidar"]
    assert raw.shape == (99, 3) and lid.shape[0] == 99 and odom.shape == (100, 3), (raw.shape, lid.shape)
    out = os.path.join(HERE, "localize_data.npz")
    np.savez_compressed(out, odom=odom, odom_raw=raw, map_param=map_param(d), n_frames=np.int32(99))
    print("wrote", out, os.path.getsize(out), "bytes")


def _tests_on_path():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def survey_one(name):
    _tests_on_path()
    import importlib
    import fa_logs
    from oracle import oracle
    oracle.build()
    lsdmod = importlib.import_module("linesegmentdetector-slam_amd")
    log = read_log(name)
    key = name.split("_")[0]
    m = np.load(os.path.join(HERE, "maps.npz"))[key]
    n = int(log["n_frames"])
    run = fa_logs.replay(oracle, lsdmod, (m, log["map_param"], log["lidar"][:n], log["odom"]))
    rec = fa_logs.summary(run, log["map_param"], log["real_pos"], log["recorded"])
    print(name, json.dumps(rec), flush=True)
    return name, rec


def select(survey):
    """Three logs per key that are not fixtures yet (data1 is): the longest, the one with the most resets after its first fix, the one
    with the largest n_kept; a tie, or a log already chosen, goes to the next by the same rule and then to the lowest number."""
    chosen = []
    for key, (_, n) in KEYS.items():
        names = ["%s_%d" % (key, i) for i in range(2, n + 1)]
        for field in ("frames", "resets_after_first_fix", "max_n_kept"):
            order = sorted(names, key=lambda nm: (-survey[nm][field], int(nm.split("_")[1])))
            chosen.append(next(nm for nm in order if nm not in chosen))
    return chosen


def survey():
    import multiprocessing as mp
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(survey_one, all_logs(), chunksize=1))
    out = {k: out[k] for k in all_logs()}
    json.dump(dict(logs=out, selected=select(out)), open(SURVEY, "w"), indent=1)
    print("wrote", SURVEY, "selected:", select(out))


def main(argv):
    if argv[:1] == ["survey"]:
        return survey()
    if argv[:1] == ["pack"]:
        for name in argv[1:]:
            pack(name)
        return
    pack_data()
    for name in ("f3key", "f4key"):
        pack(name)


if __name__ == "__main__":
    main(sys.argv[1:])
