"""One GICP correspondence pass and one Gauss-Newton accumulation on the device (lsr_gicp_linearize: the launches of align itself)
against the oracle's neighbour search and the plain numpy linearisation of tests/gicp_numpy.py — stage by stage, so that an error a
converging solver would forgive (a wrong Hessian entry, a mis-indexed dR, a dropped tail point, a wrong neighbour, a pair count off
by a few) shows as what it is."""
import numpy as np
import pytest

import gicp_numpy as GN
from lidarslam_ros2_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [37, 64, 257, 1501]      # less than a wave, a wave, one point past a 256-thread workgroup, a ragged tail over several
X_POSE = (0.3, -0.2, 0.1, 0.05, -0.08, 0.12)
U = 2.0 ** -53


def pose_matrix(x):
    """The float matrix of the state x (rotation rounded from fp64)."""
    R, _ = GN.state(x)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R.astype(np.float32)
    T[:3, 3] = np.asarray(x[:3], np.float32)
    return T


def step_matrix():
    """3 cm / 2 mrad."""
    return pose_matrix((0.02, -0.02, 0.01, 0.0012, -0.0012, 0.001))


TRANS = {"identity": np.eye(4, dtype=np.float32), "pose": pose_matrix(X_POSE)}


class Env:
    def __init__(self):
        from oracle import oracle as O

        self.O = O
        c = synth.small_case(n_source=1501, n_keyframes=2)
        self.source, self.guess = c.source, c.guess
        self.target = synth.voxel_downsample(c.target, 0.4)
        self.nn = O.NearestNeighbour(self.target)
        self.out = GN.xform32(self.guess, self.source)
        self.oracle = {}     # trans name -> (idx, d2) of all 1501 points (a point's neighbour does not depend on the others)
        self.gates = {}      # (trans name, gate name) -> metres
        for name, T in TRANS.items():
            idx, d2 = self.nn.search(self.out, T)
            self.oracle[name] = (idx, d2)
            # the tight gate: the median neighbour distance under this trans, to the centimetre -> about half of the points pair
            tight = round(float(np.sqrt(np.median(d2))), 2)
            self.gates[(name, "wide")] = 5.0
            self.gates[(name, "tight")] = tight
        self.regs, self.covs, self.cache = {}, {}, {}

    def thr2(self, gate):
        return np.float32(gate * gate)

    def reg(self, n, fresh=False, source=None):
        from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint

        if not fresh and n in self.regs:
            return self.regs[n]
        g = GeneralizedIterativeClosestPoint(device=0)
        g.setTransformationEpsilon(1e-8)
        g.setInputTarget(self.target)
        g.setInputSource(self.source[:n] if source is None else source)
        if not fresh:
            self.regs[n] = g
            self.covs[n] = (g.covariances("source"), g.covariances("target"))
        return g

    def lin(self, n, tname, gname):
        key = (n, tname, gname)
        if key not in self.cache:
            g = self.reg(n)
            g.setMaxCorrespondenceDistance(self.gates[(tname, gname)])
            self.cache[key] = g.linearize(self.guess, TRANS[tname])
        return self.cache[key]


@pytest.fixture(scope="module")
def env():
    return Env()


CASES = [(n, t, g) for n in SIZES for t in ("identity", "pose") for g in ("wide", "tight")]


def test_the_tight_gates_pair_a_part_of_the_scan(env):
    for tname in TRANS:
        gate = env.gates[(tname, "tight")]
        d2 = env.oracle[tname][1]
        frac = float((d2 < env.thr2(gate)).mean())
        print(f"trans {tname}: tight gate {gate} m pairs {frac:.3f} of 1501; the 5 m gate {float((d2 < env.thr2(5.0)).mean()):.3f}")
        assert 0.2 <= frac <= 0.8
        for g in (gate, 5.0):    # no distance sits between the float and the double square of a gate: `d2 < thr^2` has one reading
            assert np.array_equal(d2 < env.thr2(g), d2.astype(np.float64) < g * g)


@pytest.mark.parametrize("n,tname,gname", CASES)
def test_correspondences(env, n, tname, gname):
    """K6.  The search is gated: the device proves a neighbour only within the gate (cells and rows beyond it are never read), so for
    a point the oracle pairs the neighbour must be the oracle's; for a point it does not pair, nn_idx is -1 or some target point
    beyond the gate (what the next outer iteration is offered as a seed), and the record is empty."""
    r = env.lin(n, tname, gname)
    gate = env.gates[(tname, gname)]
    thr2 = env.thr2(gate)
    assert np.array_equal(r["out"], env.out[:n])                    # gicp_begin_align_kernel; numpy float32 == xform_rn, bit for bit
    idx, d2 = (a[:n] for a in env.oracle[tname])
    paired = d2 < thr2
    assert np.array_equal(r["valid"], paired.astype(np.int32))
    assert np.array_equal(r["nn_idx"][paired], idx[paired])
    rest = r["nn_idx"][~paired]
    print(f"n {n} {tname} {gname}: {int(paired.sum())} paired; of {rest.size} unpaired {int((rest == -1).sum())} have no neighbour, "
          f"{int((rest == idx[~paired]).sum())} the oracle's")
    assert np.all((rest >= -1) & (rest < env.target.shape[0]))
    moved = GN.xform32(TRANS[tname], r["out"][~paired][rest >= 0])
    diff = env.target[rest[rest >= 0]] - moved
    assert np.all((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2] >= thr2)
    if paired.all():
        assert np.array_equal(r["nn_idx"], idx)
    assert np.array_equal(r["q"], np.where(paired[:, None], env.target[np.maximum(r["nn_idx"], 0)], np.float32(0)))
    assert r["m"] == int(paired.sum())
    # the pair counters are never reset between outer iterations: the count is their total less the total remembered before
    g = env.reg(n)
    g.setMaxCorrespondenceDistance(gate)
    for seeds in (True, True, False):
        assert g.linearize(env.guess, TRANS[tname], use_seeds=seeds)["m"] == r["m"]


def test_no_pair_anywhere_in_two_waves(env):
    """128 consecutive points (two whole waves of the one-thread-per-point pass, 32 of the sixteen-lanes-per-point one) moved out
    of reach: nothing of them pairs, the count drops by what paired before, every other row is untouched."""
    base = env.lin(1501, "identity", "wide")
    src = env.source.copy()
    src[256:384] += np.float32(500.0)
    g = env.reg(1501, fresh=True, source=src)
    g.setMaxCorrespondenceDistance(5.0)
    r = g.linearize(env.guess, TRANS["identity"])
    gone = np.zeros(1501, bool)
    gone[256:384] = True
    assert not r["valid"][gone].any() and np.array_equal(r["valid"][~gone], base["valid"][~gone])
    assert r["m"] == base["m"] - int(base["valid"][gone].sum()) and base["valid"][gone].sum() > 100
    assert not r["M6"][gone].any() and not r["q"][gone].any()
    for k in ("out", "nn_idx", "q"):
        assert np.array_equal(r[k][~gone], base[k][~gone]), k
    # a Mahalanobis matrix also depends on the point's own covariance, i.e. on its 20 neighbours IN THE SCAN: where that is
    # unchanged, so are the bits
    same = ~gone & (g.covariances("source") == env.covs[1501][0]).all(axis=(1, 2))
    assert same.sum() > 1000
    assert np.array_equal(r["M6"][same], base["M6"][same])


@pytest.mark.parametrize("n,tname,gname", CASES)
def test_mahalanobis_matrices(env, n, tname, gname):
    """|M6 - ref|max <= 1e-10 |ref|max per pair: the regularised covariances have eigenvalues (1e-3, 1, 1), so S = C2 + R C1 R^T has
    eigenvalues in [2e-3, 2] and condition <= 1e3; a cofactor inverse in fp64 is good to a few cond * 2^-53 ~ 1e-12."""
    r = env.lin(n, tname, gname)
    C1, C2 = env.covs[n]
    Rm = (TRANS[tname].astype(np.float64) @ env.guess.astype(np.float64))[:3, :3]   # gicp_begin_outer_pre: fp64 product of the floats
    v = r["valid"] != 0
    ref = np.asarray(GN.mahalanobis(C1[v], C2[r["nn_idx"][v]], Rm), np.float64)
    got = GN.sym6_to_33(r["M6"][v])
    err = np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    print(f"n {n} {tname} {gname}: worst relative error of M {err.max():.2e}")
    assert err.max() <= 1e-10
    assert not r["M6"][~v].any()


@pytest.mark.parametrize("n,tname,gname", CASES)
def test_state(env, n, tname, gname):
    r = env.lin(n, tname, gname)
    T = TRANS[tname].astype(np.float64)
    x_ref = np.array([T[0, 3], T[1, 3], T[2, 3], np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0])])
    assert np.abs(r["x6"] - x_ref).max() <= 1e-15
    R, dR = GN.state(r["x6"])
    # each rotation entry: at most two products of up to three fp32 sines / cosines
    assert np.abs(r["T12"][:, :3].astype(np.float64) - R).max() <= 8 * 2.0 ** -24
    assert np.array_equal(r["T12"][:, 3], r["x6"][:3].astype(np.float32))
    assert np.abs(r["dR"] - dR).max() <= 1e-14
    if tname == "pose":     # every entry that can be non-trivial is
        assert np.abs(r["x6"] - np.array(X_POSE)).max() < 1e-6
        assert (np.abs(dR) > 1e-3).sum() == 21     # all but dR/dphi's first column and dR/dpsi's bottom row


def _reference_sums(r):
    """The 28 sums from the device's own out, T12, q, M6 and dR: the fp32 residual reproduced operation for operation (float
    transform, float subtraction, then widened), everything after it in longdouble."""
    v = r["valid"] != 0
    p = r["out"][v]
    res = (GN.xform32(r["T12"], p) - r["q"][v]).astype(np.float64)
    return GN.system(res, p.astype(np.float64), GN.sym6_to_33(r["M6"][v]), r["dR"]), (res, p)


@pytest.mark.parametrize("n,tname,gname", CASES)
def test_gauss_newton_sums(env, n, tname, gname):
    """K7.  |sums28[k] - ref[k]| <= (m + 16) 2^-53 abs_ref[k]: any-order fp64 summation of m terms plus the rounding of one term's
    own products."""
    r = env.lin(n, tname, gname)
    (ref, abs_ref), _ = _reference_sums(r)
    m = r["m"]
    assert m >= 4
    err = np.abs(np.asarray(r["sums28"], GN.LD) - ref)
    bar = (m + 16) * U * abs_ref
    ratio = np.asarray(err / np.maximum(bar, np.finfo(np.float64).tiny), np.float64)
    print(f"n {n} {tname} {gname}: m {m}, worst |err| / bar {ratio.max():.3f} at sum {int(ratio.argmax())}; "
          f"relative to the sums {float((err / abs_ref).max()):.2e}")
    assert np.all(err <= bar), [(k, float(err[k]), float(bar[k])) for k in np.nonzero(err > bar)[0]]
    assert np.all(abs_ref[[0, 7, 13, 18, 22, 25, 27]] > 0)


SEED_CASES = [("identity", TRANS["identity"], step_matrix() @ TRANS["identity"]),
              ("pose", TRANS["pose"], step_matrix() @ TRANS["pose"]),
              ("far", TRANS["identity"], TRANS["pose"])]    # most seeds wrong: the ball search has to leave its seed cells


@pytest.mark.parametrize("name,A,B", SEED_CASES, ids=[c[0] for c in SEED_CASES])
@pytest.mark.parametrize("gname", ["wide", "tight"])
def test_seeded_search_is_exact(env, name, A, B, gname):
    """The neighbours of a previous pass as seeds change nothing: the same pairs, matrices and sums as the unseeded search."""
    gate = env.gates[("pose" if name != "identity" else "identity", gname)]
    g1, g2 = env.reg(1501, fresh=True), env.reg(1501, fresh=True)
    for g in (g1, g2):
        g.setMaxCorrespondenceDistance(gate)
    g1.linearize(env.guess, A)
    seeded = g1.linearize(env.guess, B, use_seeds=True)
    plain = g2.linearize(env.guess, B)
    v = plain["valid"] != 0
    print(f"{name} {gname}: m {plain['m']}; nn_idx differs on {int((seeded['nn_idx'] != plain['nn_idx']).sum())} rows, "
          f"{int((seeded['nn_idx'] != plain['nn_idx'])[v].sum())} of them paired")
    assert plain["m"] >= 100
    assert np.array_equal(seeded["valid"], plain["valid"])
    assert np.array_equal(seeded["nn_idx"][v], plain["nn_idx"][v])
    for k in ("M6", "q", "sums28"):
        assert np.array_equal(seeded[k], plain[k]), k
    assert seeded["m"] == plain["m"]


def test_fewer_than_four_pairs(env):
    idx, d2 = env.oracle["identity"]
    g = env.reg(1501, fresh=True, source=env.source + np.float32(500.0))
    g.setMaxCorrespondenceDistance(0.5)
    r = g.linearize(env.guess)
    assert r["m"] == 0 and not r["valid"].any()
    keep = np.argsort(d2, kind="stable")[:3]
    assert d2[keep].max() < np.float32(0.25)
    src = env.source + np.float32(500.0)
    src[keep] = env.source[keep]
    g.setInputSource(src)
    r = g.linearize(env.guess)
    assert r["m"] == 3 and np.array_equal(np.nonzero(r["valid"])[0], np.sort(keep))


def test_too_few_points_is_aligns_status(env):
    from lidarslam_ros2_amd import _capi

    g = env.reg(1501, fresh=True, source=env.source[:10])
    with pytest.raises(_capi.RegistrationError) as ei:
        g.linearize(env.guess)
    assert ei.value.status == -8


def test_linearize_leaves_nothing_behind(env):
    fresh = env.reg(1501, fresh=True)
    fresh.align(env.guess)
    g = env.reg(1501, fresh=True)
    g.linearize(env.guess)
    g.linearize(env.guess, TRANS["pose"], use_seeds=True)
    g.linearize(env.guess, step_matrix())
    g.align(env.guess)
    assert np.array_equal(g.getFinalTransformation(), fresh.getFinalTransformation())
    a, b = g.last_result, fresh.last_result
    assert a["iterations"] == b["iterations"] and a["n_correspondences"] == b["n_correspondences"]
    assert a["n_evaluations"] == b["n_evaluations"] and a["score"] == b["score"] and a["converged"] == b["converged"]
    assert b["iterations"] >= 2
