"""Tilted worlds for the NDT tests.  Test infrastructure only (a plain module, not a conftest).

Every other NDT input of the suite is yaw-only: synth.trajectory_pose has roll = pitch = 0.  Here synth.small_case is re-posed by
a rigid frame W (target' = W target, guess' = W guess, truth' = W truth, the source stays), so that the guess carries roll and
pitch and — for a negative roll — leaves Eigen's eulerAngles(0,1,2) on its alias branch with all three angles near +-pi
(csrc/ndt.hip: euler012_f).  The registration problem is the same one in another frame: it converges like the flat one.

blocks() / assert_blocks() compare one derivative pass block by block: the rotation block of the Hessian is ~400 times the
translation block on this scene (and |g_rot| ~ 30 |g_trans|), so a bar relative to the whole matrix hides the translation entries."""
import functools

import numpy as np

from lidarslam_ros2_amd import synth

from ndt_variants import DERIV_TOL, SCORE_TOL   # the project's bars for one pass against the oracle

RES = 3.0
N_SOURCE = 2000

# name -> (x, y, z, yaw, roll, pitch) of W = synth.pose_matrix(x, y, z, yaw, roll=, pitch=); flipped: the guess decomposes on the
# alias branch.  Euler angles of guess' by the oracle: flat (0, 0, 0.006), roll+ (0.06, 0.04, 0.006), roll- (3.0816, 3.1016, -3.1357),
# far (3.0816, -3.1016, -0.6357), steep (0.3, -0.4, -1.694), tiny- (3.1416, 3.1416, -0.0357)
FRAMES = {
    "flat":  (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "roll+": (0.0, 0.0, 0.0, 0.0, 0.06, 0.04),
    "roll-": (0.0, 0.0, 0.0, 0.0, -0.06, 0.04),
    "far":   (12.0, -7.0, 3.0, 2.5, -0.06, -0.04),
    "steep": (12.0, -7.0, 3.0, -1.7, 0.3, -0.4),
    "tiny-": (0.0, 0.0, 0.0, 3.1, -1e-5, 2e-5),
}
FLIPPED = ("roll-", "far", "tiny-")
FRAME_NAMES = tuple(FRAMES)

SIZES = (1, 63, 64, 65, 129, 2000)     # one chunk of 64 short, one chunk, one over, one over a 128-point quad workgroup
# Inputs replaced because the host emulation itself misses a tenth of the bars there (tests/test_ndt_tilted_cpu.py, the guard):
# frame "far", 65 points, pose form: g_t 2.19e-6 against 2e-6 (the pose-form transform differs from the oracle's by an ulp of fp32 in
# a frame 14 m from the origin with all angles near pi, ~1e-4 absolute in g_t, and 65 points give a |g_t| of only 57); 193 points are
# one over a chunk as well (2.5e-7 there).
REPLACED_SIZES = {("far", 65): 193}
HESSIAN_FORMS = (True, False, 2)      # 2: the fused form (score and gradient of a gradient-only pass, Hessian of a full one)
POSE_OFFSET = np.array([0.2, -0.15, 0.05, 0.01, -0.015, 0.02])
SCHEDULES = ((0.01, 35), (1e-6, 30))   # (transformation epsilon, maximum iterations): the reference's and the tight one

# the 1e-4 small-angle snap of the angle tables, on or off per axis: 0 and 5e-5 snap, 2e-4 does not
SNAP_ANGLES = ((0.0, 0.0, 0.0), (5e-5, 5e-5, 5e-5), (-5e-5, -5e-5, -5e-5), (5e-5, -5e-5, 0.0),       # all snapped
               (2e-4, 2e-4, 2e-4), (-2e-4, 2e-4, -2e-4),                                              # none snapped
               (2e-4, 0.0, 0.0), (0.0, -2e-4, 0.0), (0.0, 0.0, 2e-4),                                 # one axis unsnapped
               (5e-5, 2e-4, 2e-4), (2e-4, -5e-5, -2e-4), (-2e-4, -2e-4, 5e-5),                        # one axis snapped
               (2e-4, 5e-5, 0.0), (-5e-5, 0.0, -2e-4))


def frame_matrix(name):
    x, y, z, yaw, roll, pitch = FRAMES[name]
    return synth.pose_matrix(x, y, z, yaw, roll=roll, pitch=pitch)


def repose(case, W):
    """(target', guess', truth') of `case` seen from frame W: fp64 products, target' and guess' rounded to fp32 once."""
    W = np.asarray(W, np.float64)
    target = (case.target.astype(np.float64) @ W[:3, :3].T + W[:3, 3]).astype(np.float32)
    guess = (W @ case.guess.astype(np.float64)).astype(np.float32)
    truth = W @ np.asarray(case.truth, np.float64)
    return target, guess, truth


@functools.lru_cache(maxsize=None)
def base_case():
    return synth.small_case(n_source=N_SOURCE, n_keyframes=3)


class Tilted:
    """One frame: the re-posed inputs and, built once, the oracle's voxel grid over target'."""

    def __init__(self, name):
        self.name = name
        c = base_case()
        self.source = c.source
        self.target, self.guess, self.truth = repose(c, frame_matrix(name))
        self._grid = None
        self._aligned = {}

    def grid(self, O):
        if self._grid is None:
            self._grid = O.VoxelGridCovariance(self.target, RES)
        return self._grid

    def poses(self, O):
        """The two poses of a derivative pass: [("matrix", p, T = guess'), ("pose", p + POSE_OFFSET, None)]."""
        p0 = O.matrix_to_pose(self.guess)
        return [("matrix", p0, self.guess), ("pose", p0 + POSE_OFFSET, None)]

    def oracle_align(self, O, eps, max_iter, **kw):
        key = (eps, max_iter, tuple(sorted(kw.items())))
        if key not in self._aligned:
            self._aligned[key] = O.ndt_align(self.grid(O), self.source, self.guess, resolution=RES, trans_eps=eps,
                                             max_iterations=max_iter, **kw)
        return self._aligned[key]


@functools.lru_cache(maxsize=None)
def tilted(name):
    return Tilted(name)


def snap_poses(O):
    """Pose-form poses on frame "flat": the translation of the offset pose, each angle on or off the 1e-4 snap."""
    p0 = O.matrix_to_pose(tilted("flat").guess)
    return [np.r_[p0[:3] + POSE_OFFSET[:3], a] for a in SNAP_ANGLES]


def oracle_pass(O, w, n, p, T, form, **kw):
    """O.ndt_derivatives on the first n source points in the shape of Hessian form `form` (False: H stays zero)."""
    return O.ndt_derivatives(w.grid(O), w.source[:n], p, T=T, compute_hessian=bool(form), resolution=RES, **kw)


def emu_pass(emu, p, T, form):
    """The host emulation in the shape of Hessian form `form`; 2 = score and gradient of a gradient-only pass, H of a full one."""
    if form == 2:
        s, g, _ = emu.derivatives(p, T=T, with_hessian=False)
        return s, g, emu.derivatives(p, T=T, with_hessian=True)[2]
    return emu.derivatives(p, T=T, with_hessian=bool(form))


BLOCKS = ("score", "g_t", "g_r", "H_tt", "H_tr", "H_rr")


def _split(s, g, H):
    g, H = np.asarray(g, np.float64), np.asarray(H, np.float64)
    return {"score": np.array([float(s)]), "g_t": g[:3], "g_r": g[3:], "H_tt": H[:3, :3],
            "H_tr": np.concatenate([H[:3, 3:].ravel(), H[3:, :3].ravel()]), "H_rr": H[3:, 3:]}


def blocks(got, ref):
    """The six relative differences of (score, g, H) `got` against `ref`: score relative; g[:3], g[3:], H[:3,:3], H[:3,3:] (with its
    transpose) and H[3:,3:] each over the largest reference entry of the block.  A block whose reference is all zero gives 0.0 if
    `got` is all zero there too and inf otherwise."""
    a, b = _split(*got), _split(*ref)
    out = {}
    for k in BLOCKS:
        den = np.abs(b[k]).max()
        num = np.abs(a[k] - b[k]).max()
        if not np.all(np.isfinite(a[k])):
            out[k] = float("inf")
        elif den == 0.0:
            out[k] = 0.0 if num == 0.0 else float("inf")
        else:
            out[k] = float(num / den)
    return out


def assert_blocks(got, ref, margin=1.0, label=None, worst=None):
    """Hold (score, g, H) `got` to `ref` block by block: SCORE_TOL on the score, DERIV_TOL on each of the five other blocks, times
    `margin` (< 1 tightens).  Returns the six values; `worst` (a dict) collects the largest value seen per block."""
    d = blocks(got, ref)
    for k in BLOCKS:
        bar = (SCORE_TOL if k == "score" else DERIV_TOL) * margin
        assert d[k] <= bar, (label, k, d[k], bar, d)
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), d[k])
    return d


def fmt(worst):
    return "  ".join("%s %.1e" % (k, worst.get(k, 0.0)) for k in BLOCKS)


TRUNCATED_FRAMES = ("roll-", "roll+")   # registrations stopped after every Newton step, on both branches of the decomposition


def n_passes(ref):
    """Derivative passes of an O.ndt_align result: what the device reports as n_evaluations."""
    return ref["n_evals"] + ref["n_evals_grad"] + ref["n_hessian_recompute"]


def sizes(name):
    """The source prefixes of the block-by-block derivative tests on frame `name`; each runs both poses and the three Hessian forms."""
    return tuple(REPLACED_SIZES.get((name, n), n) for n in SIZES)
