"""The launch variants of the NDT derivative pass and the registration tolerances the GPU tests share.  Test infrastructure only.

VARIANTS: (quad, workgroup, table_mode[, split]) — quad: 1 = four lanes per point (workgroup = points per workgroup: 0 auto / 64 /
128), 0 = lane kernel, one lane per point (workgroup = threads: 512 / 1024); table mode: 0 dense global, 1 compact global, 2 LDS;
a fourth entry: split = 1 — two waves per chunk in the 512-thread lane kernel."""

POSE_T_TOL = 1e-3   # metres   (north_star)
POSE_R_TOL = 1e-4   # radians  (north_star)
SCORE_TOL = 1e-5    # one derivative pass against the oracle: score, relative
DERIV_TOL = 2e-5    # ... gradient and Hessian, relative to the largest entry of what is compared

VARIANTS = [(1, 0, 2), (1, 0, 0), (1, 0, 1), (1, 64, 2), (0, 1024, 0), (0, 1024, 1), (0, 1024, 2), (0, 512, 0), (0, 512, 2),
            (0, 512, 0, 1), (0, 512, 1, 1), (0, 512, 2, 1)]


def tune(ndt, v):
    """Select launch variant `v` of VARIANTS on a registration object."""
    quad, workgroup, table_mode = v[:3]
    ndt.setTuning(workgroup=workgroup, table_mode=table_mode, quad=quad, split=(v[3] if len(v) > 3 else 0))
