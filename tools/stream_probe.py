#!/usr/bin/env python3
"""Developer probe: the per-tick cost of the resumable loop (Localizer.step -> lsd_enqueue_localize_resume_device) on the data/ log of
tests/golden/, to set beside tools/localize_probe.py's one-call replay.

S robots (S = 1, 19, 256 by default) step one frame per call for TICKS ticks, robot s on the log from frame (7 s) mod (99 - TICKS), as
localize_probe.py staggers its sequences.  A tick is timed whole, from a warm Localizer:
  --input host       (default) Localizer.step from host arrays: the upload of the raw frames, the ingest launch (k_ingest: the
                     infinite-range filter), FeatureScan of the S scans, the three FeatureAssociation launches, and the read-back of the
                     tick's states and reports (one synchronisation);
  --input device     Localizer.step_device from (range, angle) pairs already on the device, then the caller's synchronisation: no upload,
                     no read-back (the frames of a tick are gathered on the device before the clock starts);
  --input laserscan  the same from float32 ranges and (angle_min, angle_increment) per message.
us_host_filter_median is the host's infinite-range filter (lidar_frames_batch) on the tick's frames, measured beside the tick: the cost
Localizer.step contained before the filter moved onto the device.  One JSON line per S.

--map-update: the map side instead, on the f3key map and log.  For every S, from "the OccupancyGrid is on the device" to "the first tick
on the new map has finished" (the caller's synchronisation), --reps times per run, --runs runs of each path alternating in one session:
  path host    what the map callback cost before the device-side update: the grid's download, mapCallback (three blocking host calls),
               Localizer.set_map (the fp64 cache and the lines uploaded again), step_device;
  path device  Localizer.set_map_device on a side stream, step_device on the current one: no host round trip, no synchronisation.
Each run also steps --ticks ticks with ONE update a third of the way in, an event recorded behind every tick, and reports the longest and
the median gap between two consecutive ticks' completions (us_gap_max / us_gap_median; the device clock).  One JSON line per S, path and
run, then one summary line per S and path: the median of the runs' medians and, as spread, their range.  The probe reports; it asserts
nothing.

--maps M[,M...]: a fleet on M maps (the maps of the three logs data, f3key, f4key, cycled), the S robots dealt to the maps in M equal
blocks (the first S mod M blocks one robot larger), every robot on its map's log.  A tick -- step_device from pairs on the device, then
the caller's synchronisation -- is timed on two paths, --runs runs of --ticks ticks each, alternating in one session:
  path fleet       ONE FleetLocalizer tick for all S robots (lsd_enqueue_feature_scan_maps_device, lsd_enqueue_localize_resume_maps_device);
  path localizers  M Localizers, one per map with its block of robots, ticked one after the other on the same stream: the single-map
                   entries, what such a fleet cost before.  At M = 1 this is Localizer itself: the pair shows what the table costs.
One JSON line per S, M, path and run, then a summary line per S, M and path (the median of the runs' medians, their range as spread).
Usage: tools/stream_probe.py [--robots 1,19,256] [--ticks 60] [--warm 3] [--input host|device|laserscan]
       tools/stream_probe.py --map-update [--robots 1,19,256] [--ticks 30] [--reps 5] [--runs 3]
       tools/stream_probe.py --maps 1,3,8 [--robots 24,256] [--ticks 30] [--runs 3]"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fa_restatement as fr

lsd = importlib.import_module("linesegmentdetector-slam_amd")


def map_update(args):
    m, mp, lid, odom = fr.load_log("f3key")
    rows, cols = m.shape
    p = [float(v) for v in mp]
    grid = np.where(m == 0, -1, np.where(m == 255, 0, 100)).astype(np.int8)            # unknown / free / occupied cells
    d_grid, d_lid, d_od = torch.from_numpy(grid).cuda(), torch.from_numpy(lid).cuda(), torch.from_numpy(odom).cuda()
    ctx, side, T = lsd.Context(0), torch.cuda.Stream(), args.ticks
    for S in (int(v) for v in args.robots.split(",")):
        starts = np.array([(7 * s) % (len(lid) - T - args.reps) for s in range(S)])
        od0 = odom[starts].copy(); od0[:, 0] = 0.0
        loc = lsd.Localizer.from_occupancy_grid(grid.reshape(-1), cols, rows, p[2], p[3], p[4], S, odom0=od0, ctx=ctx)
        loc.reserve_map(cols, rows)
        d_starts = torch.from_numpy(starts).cuda()
        ins = [(d_lid[d_starts + t][:, None].contiguous(), d_od[d_starts + t + 1][:, None].contiguous()) for t in range(T + args.reps)]

        def host_update():
            g = d_grid.cpu().numpy()                                     # the grid is on the device: the host path starts with its download
            _, mc, LSD = lsd.mapCallback(g.reshape(-1), cols, rows, p[2], ctx=ctx)
            loc.set_map(mc, LSD.linesInfo, p)
            return LSD.len_linesInfo

        def device_update():
            loc.set_map_device(d_grid, cols, rows, p[2], p[3], p[4], stream=side)

        for update in (host_update, device_update):                      # warm: code loaded, both slots and every workspace sized
            update(); loc.step_device(*ins[0]); torch.cuda.synchronize()
        n_lines = host_update()
        meds = {"host": [], "device": []}
        for run in range(args.runs):
            for path, update in (("host", host_update), ("device", device_update)):
                loc.reset(range(S), odom0=od0)
                torch.cuda.synchronize()
                ts = []
                for r in range(args.reps):
                    t0 = time.perf_counter()
                    update()
                    loc.step_device(*ins[r])
                    torch.cuda.synchronize()                             # the caller's own: the first tick on the new map has finished
                    ts.append(time.perf_counter() - t0)
                evs = []
                for t in range(T):
                    if t == T // 3:
                        update()
                    loc.step_device(*ins[args.reps + t])
                    evs.append(torch.cuda.Event(enable_timing=True)); evs[-1].record()
                torch.cuda.synchronize()
                gaps = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(T - 1)]) * 1e3
                ts = np.array(ts) * 1e6
                meds[path].append(float(np.median(ts)))
                print(json.dumps(dict(mode="map-update", robots=S, path=path, run=run + 1, map="f3key", map_lines=n_lines, reps=args.reps,
                                      us_update_to_tick_median=float(np.median(ts)), us_update_to_tick_min=float(ts.min()),
                                      us_update_to_tick_max=float(ts.max()), ticks=T, us_gap_max=float(gaps.max()), gap_at=int(gaps.argmax()) + 1,
                                      update_before_tick=T // 3, us_gap_median=float(np.median(gaps)))), flush=True)
        for path, v in meds.items():
            print(json.dumps(dict(mode="map-update", robots=S, path=path, summary=True, runs=args.runs, us_update_to_tick=float(np.median(v)),
                                  spread=float(max(v) - min(v)))), flush=True)
    ctx.close()


def fleet(args):
    ctx, T = lsd.Context(0), args.ticks
    logs = []
    for name in fr.LOGS:
        m, mp, lid, odom = fr.load_log(name)
        mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
        ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        logs.append(dict(name=name, map=(mc, ml, mp), lid=lid, odom=odom, d_lid=torch.from_numpy(lid).cuda(), d_od=torch.from_numpy(odom).cuda()))
    for S in (int(v) for v in args.robots.split(",")):
        for M in (int(v) for v in args.maps.split(",")):
            sizes = [S // M + (1 if i < S % M else 0) for i in range(M)]
            if min(sizes) < 1:
                continue
            groups, map_of = [], []
            for i, n in enumerate(sizes):
                lg = logs[i % len(logs)]
                starts = np.array([(7 * s) % (len(lg["lid"]) - T - args.warm) for s in range(n)])
                od0 = lg["odom"][starts].copy(); od0[:, 0] = 0.0
                d_starts = torch.from_numpy(starts).cuda()
                ins = [(lg["d_lid"][d_starts + t][:, None].contiguous(), lg["d_od"][d_starts + t + 1][:, None].contiguous())
                       for t in range(T + args.warm)]
                groups.append(dict(log=lg, od0=od0, ins=ins, loc=lsd.Localizer(*lg["map"], n, odom0=od0, ctx=ctx)))
                map_of += [i] * n
            od0 = np.concatenate([g["od0"] for g in groups])
            fl = lsd.FleetLocalizer([g["log"]["map"] for g in groups], map_of, odom0=od0, ctx=ctx)
            all_ins = [(torch.cat([g["ins"][t][0] for g in groups]), torch.cat([g["ins"][t][1] for g in groups])) for t in range(T + args.warm)]

            def tick_fleet(t):
                return [fl.step_device(*all_ins[t])]

            def tick_localizers(t):
                return [g["loc"].step_device(*g["ins"][t]) for g in groups]

            def restart():
                fl.reset(range(S), odom0=od0)
                for g in groups:
                    g["loc"].reset(range(g["loc"].n_robots), odom0=g["od0"])
            paths = (("fleet", tick_fleet), ("localizers", tick_localizers))
            for _, tick in paths:                                        # warm: staging, workspace and table sized, code loaded
                for t in range(args.warm):
                    tick(t)
            torch.cuda.synchronize()
            meds = {name: [] for name, _ in paths}
            for run in range(args.runs):
                for name, tick in paths:
                    restart()
                    torch.cuda.synchronize()
                    ts, kept = [], []
                    for t in range(T):
                        t0 = time.perf_counter()
                        outs = tick(args.warm + t)
                        torch.cuda.synchronize()                         # the caller's own
                        ts.append(time.perf_counter() - t0)
                        kept.append(np.concatenate([o[1].cpu().numpy().reshape(-1).view(lsd.FA_REPORT_DTYPE)["n_kept"] for o in outs]))
                    ts, kept = np.array(ts) * 1e6, np.concatenate(kept)
                    meds[name].append(float(np.median(ts)))
                    print(json.dumps(dict(mode="fleet", robots=S, maps=M, path=name, run=run + 1, ticks=T, us_per_tick_median=float(np.median(ts)),
                                          us_per_tick_min=float(ts.min()), us_per_tick_p90=float(np.percentile(ts, 90)),
                                          map_lines=[len(g["log"]["map"][1]) for g in groups], kept_mean=float(kept.mean()),
                                          kept_max=int(kept.max()))), flush=True)
            for name, v in meds.items():
                print(json.dumps(dict(mode="fleet", robots=S, maps=M, path=name, summary=True, runs=args.runs, us_per_tick=float(np.median(v)),
                                      spread=float(max(v) - min(v)))), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="1,19,256")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--input", choices=("host", "device", "laserscan"), default="host")
    ap.add_argument("--map-update", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--maps", default=None)
    args = ap.parse_args()
    if args.map_update:
        return map_update(args)
    if args.maps:
        return fleet(args)
    m, mp, lid, odom = fr.load_log("data")
    ctx = lsd.Context(0)
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
    ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    T = args.ticks
    for S in (int(v) for v in args.robots.split(",")):
        starts = np.array([(7 * s) % (len(lid) - T) for s in range(S)])
        od0 = odom[starts].copy(); od0[:, 0] = 0.0                       # the driver's Odom[0].x = 0
        loc = lsd.Localizer(mc, ml, mp, S, odom0=od0, ctx=ctx)
        frame = lambda t: (lid[starts + t][:, None], odom[starts + t + 1][:, None])
        if args.input != "host":
            d_lid, d_od, d_starts = torch.from_numpy(lid).cuda(), torch.from_numpy(odom).cuda(), torch.from_numpy(starts).cuda()
            d_rg = d_lid[..., 0].float().contiguous()
            d_ami = torch.tensor([-3.12414, 0.0174533], dtype=torch.float32, device="cuda").expand(S, 1, 2).contiguous()

        def tick(t, a):
            if args.input == "host":
                return loc.step(*a)[1]["n_kept"], None
            od = d_od[d_starts + t + 1][:, None]
            src = dict(lidar=d_lid[d_starts + t][:, None]) if args.input == "device" else dict(ranges=d_rg[d_starts + t][:, None], angle_min_inc=d_ami)
            torch.cuda.synchronize()                                     # the tick's inputs are on the device
            t0 = time.perf_counter()
            out = loc.step_device(odom=od, **src)
            torch.cuda.synchronize()                                     # the caller's own
            dt = time.perf_counter() - t0
            return out[1].cpu().numpy().reshape(-1).view(lsd.FA_REPORT_DTYPE)["n_kept"], dt
        for t in range(args.warm):                                       # warm: staging and workspace sized, code loaded
            tick(t, frame(t))
        loc.reset(range(S), odom0=od0)
        torch.cuda.synchronize()
        ts, tf, kept = [], [], []
        for t in range(T):
            a = frame(t)
            t0 = time.perf_counter()
            k, dt = tick(t, a)
            ts.append(time.perf_counter() - t0 if dt is None else dt)
            kept.append(k)
            t0 = time.perf_counter()
            lsd.lidar_frames_batch(a[0])                                 # the host's infinite-range filter alone (no longer part of the tick)
            tf.append(time.perf_counter() - t0)
        ts, tf = np.array(ts) * 1e6, np.array(tf) * 1e6
        kept = np.concatenate(kept)
        print(json.dumps(dict(robots=S, input=args.input, ticks=T, map_lines=len(ml), us_per_tick_median=float(np.median(ts)), us_per_tick_min=float(ts.min()),
                              us_per_tick_p90=float(np.percentile(ts, 90)),
                              us_host_filter_median=float(np.median(tf)), frames_per_s=S / float(np.median(ts)) * 1e6,
                              kept_mean=float(kept.mean()), kept_max=int(kept.max()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
