"""TEST INFRASTRUCTURE: the malformed-argument table of the record-buffer entries, shared by tests/test_record_args_cpu.py (the checks of
csrc/record_args.hpp as a plain host program) and tests/test_record_args_gpu.py (the same cases through the C ABI).

The expected statuses were read off the per-entry checks as they stood BEFORE the checks were merged into one header — each entry then
carried its own copy — and not off the header: they are what a caller has always been told.
  check_layout (all pc2 entries but de-skew): point_step < 12 or not a multiple of 4; an x / y / z offset not a multiple of 4 or not
    inside point_step; an intensity offset >= 0 not a multiple of 4 or not inside point_step -> INVALID_ARGUMENT.
  lsr_deskew_pc2: the same WITHOUT the intensity test (it copies every byte outside x / y / z).
  lsr_assemble_map (out_layout), lsr_decode_pcd / lsr_load_pcd: check_layout, and two fields at one offset -> INVALID_ARGUMENT.
  ingest entries (lsr_set_input_source*, lsr_set_input_target*, the voxel filters): a null pointer with n > 0, n > INT32_MAX / 2 ->
    INVALID_ARGUMENT; no alignment demanded of the pointer.
  lsr_transform_pc2 / lsr_deskew_pc2: the same for both pointers, pointers on a 4-byte boundary, ranges equal or disjoint.
  map and PCD entries: null with n > 0, a pointer off a 4-byte boundary -> INVALID_ARGUMENT; n > INT32_MAX -> INDEX_OVERFLOW.
  frame lists: n_frames <= 0, a null array, a bad stride, a null frame with a count -> INVALID_ARGUMENT.
"""
OK, INVALID, OVERFLOW = 0, -1, -7
HALF = (2 ** 31 - 1) // 2      # the ingest, transform and de-skew entries' limit
FULL = 2 ** 31 - 1             # the map and PCD entries' limit

# (point_step, x, y, z, intensity or -1) -> (xyz part alone, whole layout, output layout)
LAYOUTS = [
    ((10, 0, 4, 8, -1), (INVALID, INVALID, INVALID)),     # point_step < 12
    ((30, 0, 4, 8, 16), (INVALID, INVALID, INVALID)),     # point_step not a multiple of 4
    ((32, 0, 4, 30, 16), (INVALID, INVALID, INVALID)),    # z off a 4-byte boundary (and outside the record)
    ((32, 2, 4, 8, 16), (INVALID, INVALID, INVALID)),     # x off a 4-byte boundary
    ((32, 0, 4, 8, 30), (OK, INVALID, INVALID)),          # intensity at 30: de-skew does not look
    ((32, 0, 4, 8, 0), (OK, OK, INVALID)),                # intensity on top of x: only a layout that is WRITTEN minds
    ((32, 0, 4, 8, 32), (OK, INVALID, INVALID)),          # intensity behind the record
    ((32, 0, 4, 32, 16), (INVALID, INVALID, INVALID)),    # z behind the record
    # one good layout per shape the suite uses (tests/test_sensor_transform_gpu.py: LAYOUTS; packed xyz)
    ((32, 0, 4, 8, 16), (OK, OK, OK)),
    ((24, 4, 12, 20, 0), (OK, OK, OK)),
    ((16, 0, 4, 8, -1), (OK, OK, OK)),
    ((48, 16, 20, 24, 40), (OK, OK, OK)),
    ((12, 0, 4, 8, -1), (OK, OK, OK)),
]
BAD_LAYOUTS = [lay for lay, (_, whole, _) in LAYOUTS if whole != OK]          # what every pc2 entry but de-skew refuses
BAD_XYZ_LAYOUTS = [lay for lay, (xyz, _, _) in LAYOUTS if xyz != OK]          # what de-skew refuses
BAD_OUT_LAYOUTS = [lay for lay, (_, _, out) in LAYOUTS if out != OK]          # what a written layout refuses

STRIDES = [(10, INVALID), (30, INVALID), (8, INVALID), (12, OK), (16, OK), (32, OK)]

P = 0x10000      # a pointer value for the host program (never dereferenced there)
# (pointer, n, limit, pointer must be 4-byte aligned) -> status
RECORDS = [
    ((0, 2, "ingest", 0), INVALID), ((0, 0, "ingest", 0), OK), ((P + 1, 2, "ingest", 0), OK),
    ((P, HALF, "ingest", 0), OK), ((P, HALF + 1, "ingest", 0), INVALID), ((P, FULL, "ingest", 0), INVALID), ((P, FULL + 1, "ingest", 0), INVALID),
    ((0, 2, "ingest", 1), INVALID), ((0, 0, "ingest", 1), OK), ((P + 1, 2, "ingest", 1), INVALID), ((P + 2, 0, "ingest", 1), INVALID),
    ((P, HALF, "ingest", 1), OK), ((P, HALF + 1, "ingest", 1), INVALID),
    ((0, 2, "map", 1), INVALID), ((0, 0, "map", 1), OK), ((P + 1, 2, "map", 1), INVALID),
    ((P, HALF + 1, "map", 1), OK), ((P, FULL, "map", 1), OK), ((P, FULL + 1, "map", 1), OVERFLOW),
    ((P + 1, FULL + 1, "map", 1), INVALID),      # the pointer is judged first
]
# 2 records of 16 bytes: (in, out, n, step) -> status
IN_OUT = [
    ((P, P, 2, 16), OK), ((P, P + 16, 2, 16), INVALID), ((P + 16, P, 2, 16), INVALID), ((P, P + 32, 2, 16), OK), ((P + 32, P, 2, 16), OK),
    ((0, P, 2, 16), INVALID), ((P, 0, 2, 16), INVALID), ((0, 0, 0, 16), OK), ((P + 1, P + 1, 2, 16), INVALID),
    ((P, P + 64, HALF + 1, 16), INVALID),
]
# (a, a_bytes, b, b_bytes) -> overlap
OVERLAP = [((P, 32, P, 32), 1), ((P, 32, P + 16, 32), 1), ((P + 16, 32, P, 32), 1), ((P, 32, P + 32, 32), 0), ((P + 32, 32, P, 32), 0),
           ((P, 0, P, 32), 0), ((P, 32, P + 8, 0), 0)]
# (stride, lists there, n_frames, [(pointer, count) ...]) -> status (, total, biggest)
FRAMES = [
    ((16, 1, 0, []), (INVALID,)), ((16, 1, -1, []), (INVALID,)), ((16, 0, 2, []), (INVALID,)),
    ((16, 1, 2, [(P, 5), (0, 3)]), (INVALID,)),                     # a null frame with a count
    ((10, 1, 2, [(P, 5), (P, 3)]), (INVALID,)),                     # stride 10
    ((16, 1, 2, [(P, HALF), (P, 1)]), (INVALID,)),                  # together above the limit
    ((16, 1, 1, [(P, HALF + 1)]), (INVALID,)),
    ((16, 1, 3, [(P, 5), (0, 0), (P + 1, 300)]), (OK, 305, 300)),   # an empty frame may be null; no alignment demanded
    ((16, 1, 2, [(P, HALF - 1), (P, 1)]), (OK, HALF, HALF - 1)),
]


def harness_lines():
    """-> (the harness's input, the lines it must print)"""
    ask, want = [], []
    for lay, st in LAYOUTS:
        ask.append("layout " + " ".join(str(v) for v in lay))
        want.append(" ".join(str(s) for s in st))
    ask.append("nolayout")
    want.append(f"{INVALID} {INVALID} {INVALID}")
    for s, st in STRIDES:
        ask.append(f"stride {s}")
        want.append(str(st))
    for name, table in (("records", RECORDS), ("inout", IN_OUT), ("overlap", OVERLAP)):
        for args, st in table:
            ask.append(name + " " + " ".join(str(v) for v in args))
            want.append(str(st))
    for (stride, lists, n, frames), st in FRAMES:
        ask.append(f"frames {stride} {lists} {n} " + " ".join(f"{p} {c}" for p, c in frames))
        want.append(" ".join(str(s) for s in st))
    return "\n".join(ask) + "\n", want
