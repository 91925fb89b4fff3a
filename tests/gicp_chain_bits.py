"""TEST INFRASTRUCTURE: the bits the GICP launch chain leaves on one fixed scenario (tests/golden/gicp_chain_bits.json).
`inputs()` and `results()` are what tests/test_gicp_gpu.py::test_chain_bits_match_the_recorded_ones compares with the fixture; run
as a script on the GPU this file prints the fixture:  python tests/gicp_chain_bits.py > tests/golden/gicp_chain_bits.json
Integer and scalar results are kept in the clear (floats as hex), arrays as SHA-256 digests of their bytes."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gicp_chain_bits.json")


def _digest(a, dtype=None) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def inputs():
    """-> (the synthetic case, digests of its clouds and guess): a change in synth shows here, before any kernel runs."""
    from lidarslam_ros2_amd import synth

    c = synth.small_case(n_source=3000, n_keyframes=3)
    return c, {"source": _digest(c.source), "target": _digest(c.target), "guess": _digest(c.guess)}


def results(c) -> dict:
    """What the device makes of the case: an align, a source with far outliers, one linearize."""
    from gicp_numpy import state
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint

    g = GeneralizedIterativeClosestPoint(device=0)
    g.setMaxCorrespondenceDistance(5.0)
    g.setTransformationEpsilon(1e-8)
    g.setInputTarget(c.target)
    g.setInputSource(c.source)
    g.align(c.guess)
    out = {"T": _digest(g.getFinalTransformation(), np.float32), "it": int(g.getFinalNumIteration()),
           "fit": float(g.getFitnessScore()).hex(), "cov_src": _digest(g.covariances("source")),
           "res": {k: v for k, v in g.last_result.items() if k != "gpu_ms"}}
    # far outliers: queries the fine shells cannot prove (coarse-cell search)
    src2 = np.vstack([c.source[:500], c.source[:8] + np.float32([60.0, -45.0, 9.0])]).astype(np.float32)
    g.setInputSource(src2)
    g.align(c.guess)
    out["fit_outliers"] = float(g.getFitnessScore()).hex()
    # one correspondence pass + one Gauss-Newton accumulation at a pose with every angle non-zero, a gate that pairs a part of the scan
    x = (0.3, -0.2, 0.1, 0.05, -0.08, 0.12)
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = state(x)[0].astype(np.float32)
    P[:3, 3] = np.float32(x[:3])
    g.setInputSource(c.source[:1501])
    g.setMaxCorrespondenceDistance(1.1)
    r = g.linearize(c.guess, P)
    assert 0.2 * 1501 <= r["m"] <= 0.8 * 1501, r["m"]
    # (a neighbour is proven only within the gate: what an unpaired point is left with, -1 or a point beyond the gate, is the search's business)
    r["nn_idx"] = np.where(r["valid"] != 0, r["nn_idx"], -1).astype(np.int32)
    out["lin"] = {k: _digest(r[k]) for k in ("nn_idx", "valid", "M6", "sums28")}
    return out


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def flatten(d: dict, prefix: str = "") -> dict:
    """{"res": {"score": 1}} -> {"res.score": 1}: one name per compared field."""
    flat = {}
    for k, v in d.items():
        if isinstance(v, dict):
            flat.update(flatten(v, prefix + k + "."))
        else:
            flat[prefix + k] = v
    return flat


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    case, digests = inputs()
    print(json.dumps({"inputs": digests, "results": results(case)}, indent=1, sort_keys=True))
