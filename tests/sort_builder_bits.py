"""TEST INFRASTRUCTURE: the bits the sort-based builders leave on one fixed scenario (tests/golden/sort_builder_bits.json): the
radix target builder of the NDT voxel grid (key spaces beyond the counting sort, and forced with grid_builder=1) and both builders
of the NN hash grid behind GICP.  `inputs()` and `results()` are what
tests/test_ndt_gpu.py::test_sort_builder_bits_match_the_recorded_ones compares with the fixture; run as a script on the GPU this
file prints the fixture:  python tests/sort_builder_bits.py > tests/golden/sort_builder_bits.json
Integers and the fitness are kept in the clear (floats as hex), arrays as "dtype[shape]:SHA-256 of the bytes"; every NaN of a float
array is mapped to the one canonical quiet NaN first, so that equal digests say what np.array_equal(..., equal_nan=True) says."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sort_builder_bits.json")


def _digest(a) -> str:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.copy()
        a[np.isnan(a)] = np.nan      # whatever payload or sign a NaN carries: the canonical quiet NaN of the dtype
    return "%s%s:%s" % (a.dtype.name, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def inputs():
    """-> (the synthetic case, the target with its NaN rows, digests of the clouds and the guess): a change in synth shows here,
    before any kernel runs."""
    from lidarslam_ros2_amd import synth

    c = synth.small_case(n_source=4000, n_keyframes=4, seed=3)
    tgt = synth.as_pointxyzi(c.target)
    tgt[5::89, 1] = np.nan
    return c, tgt, {"source": _digest(c.source), "target": _digest(c.target), "target_nan": _digest(tgt), "guess": _digest(c.guess)}


def results(c, tgt) -> dict:
    """What the device makes of the case: three voxel grids with a registration each, two NN grids with their answers."""
    from lidarslam_ros2_amd import DIRECT7, GeneralizedIterativeClosestPoint, NormalDistributionsTransform

    out = {}
    for tag, res, builder in (("r1", 1.0, 0), ("r07", 0.7, 0), ("r5_forced", 5.0, 1)):
        r = NormalDistributionsTransform(device=0)
        r.setResolution(res)
        r.setTransformationEpsilon(0.01)
        r.setNeighborhoodSearchMethod(DIRECT7)
        r.setTuning(grid_builder=builder)
        r.setInputTarget(tgt)
        r.setInputSource(c.source)
        r.align(c.guess)
        d, info = r.gridDump(), r.gridInfo()
        out[tag] = {k: _digest(d[k]) for k in ("idx", "n", "mean", "icov")}
        out[tag]["T"] = _digest(r.getFinalTransformation())
        out[tag]["leaves"] = [int(info["n_leaves"]), int(info["n_valid"])]
    for tag, builder in (("nn_bucket", 0), ("nn_sort", 1)):
        g = GeneralizedIterativeClosestPoint(device=0)
        g.setTuning(grid_builder=builder)
        g.setInputTarget(c.target)
        g.setInputSource(c.source)
        idx, d2 = g.nearestNeighbors(c.guess)
        g.align(c.guess)
        out[tag] = {"idx": _digest(idx), "d2": _digest(d2), "T": _digest(g.getFinalTransformation()),
                    "cov": _digest(g.covariances("target")), "fit": float(g.getFitnessScore()).hex()}
    return out


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def flatten(d: dict, prefix: str = "") -> dict:
    """{"r1": {"idx": ...}} -> {"r1.idx": ...}: one name per compared field."""
    flat = {}
    for k, v in d.items():
        if isinstance(v, dict):
            flat.update(flatten(v, prefix + k + "."))
        else:
            flat[prefix + k] = v
    return flat


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    case, target, digests = inputs()
    print(json.dumps({"inputs": digests, "results": results(case, target)}, indent=1, sort_keys=True))
