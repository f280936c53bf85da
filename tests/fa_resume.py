"""The replay driver's frame loop (tests/fa_restatement.py: Loop) restated on a carry: the loop's variables after some number of frames,
in the form of include/lsd_hip.h's lsd_fa_carry, so that a sequence can stop after any frame and continue from the record alone.

Loop re-sums angRotate from 0 in push order before every frame (LSD/main_on_windows.cpp:125-133); the carry keeps that very running
sum and the count, so theta rounds identically.  Odometry comes one NEW row per frame (Odom[cnt_frame]); Odom[cnt_frame - 1] is the
carry's.  The first-frame test of :176 (cnt_frame == 1) is frames == 0, the sequence's own first frame, not a call's.
"""
import math

import fa_restatement as fr


class ResumableLoop:
    """frame(odom_new, ...) per frame, in any number of calls; carry() / from_carry() move the variables in and out."""

    def __init__(self, map_resol, x0=None, P0=None, odom0=(0.0, 0.0, 0.0)):
        self.resol = float(map_resol)
        rx, rP = fr.reset_state()
        self.x = [float(v) for v in x0] if x0 is not None else rx
        self.P = [[float(v) for v in r] for r in P0] if P0 is not None else rP
        self.odom = tuple(float(v) for v in odom0)
        self.ang_sum, self.ang_count, self.frames, self.is_offset = 0.0, 0.0, 0, False

    def scan_pose(self, odom_new):
        if abs(self.x[0] + 1) < 0.0001:
            return (0.0, 0.0, 0.0)
        theta = fr.fdiv(self.ang_sum, self.ang_count)            # 0/0 when no offset has been pushed, as Loop
        o1, o0 = odom_new, self.odom
        tx, ty, ta = (o1[0] - o0[0]) / self.resol, (o1[1] - o0[1]) / self.resol, fr.atand(o1[2] - o0[2])
        s, c = fr.sind(theta), fr.cosd(theta)
        return (tx * c - ty * s, ty * s + ty * c, ta)

    def last_pose(self):
        return (self.x[0], self.x[1], self.x[2])

    def finish(self, odom_new, x, P):
        self.x, self.P = x, P
        ang = x[2] - fr.atand(odom_new[2])
        if abs(ang) > 90 and self.frames == 0:
            self.is_offset = True
        if self.is_offset and ang < 0:
            ang += 360
        self.ang_sum += ang
        self.ang_count += 1
        self.frames += 1
        self.odom = tuple(float(v) for v in odom_new)

    def carry(self, dtype):
        """The variables as one record of `dtype` (FA_CARRY_DTYPE: state.x, state.P column-major, odom, sums, frames, is_offset)."""
        import numpy as np
        c = np.zeros(1, dtype)
        c["state"]["x"][0] = self.x
        c["state"]["P"][0] = np.array(self.P, np.float64).ravel(order="F")
        c["odom"][0] = self.odom
        c["ang_sum"], c["ang_count"], c["frames"], c["is_offset"] = self.ang_sum, self.ang_count, self.frames, int(self.is_offset)
        return c[0]

    @classmethod
    def from_carry(cls, rec, map_resol):
        import numpy as np
        lp = cls(map_resol)
        lp.x = [float(v) for v in rec["state"]["x"]]
        lp.P = np.asarray(rec["state"]["P"], np.float64).reshape(9, 9, order="F").tolist()
        lp.odom = tuple(float(rec["odom"][k]) for k in ("x", "y", "ang"))
        lp.ang_sum, lp.ang_count = float(rec["ang_sum"]), float(rec["ang_count"])
        lp.frames, lp.is_offset = int(rec["frames"]), bool(rec["is_offset"])
        return lp


def same_float(a, b):
    """Bitwise equality of two floats (NaN equals NaN)."""
    return a == b or (math.isnan(a) and math.isnan(b))
