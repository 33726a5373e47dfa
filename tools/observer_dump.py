#!/usr/bin/env python3
"""Everything the three run observers hand back, for four short runs, as one .npz — to set two builds of the library against
each other bit for bit.

    GAMD_LIB=/path/to/libgamd_hip.so python tools/observer_dump.py out.npz      (one process per library: GAMD_LIB is read
    python tools/observer_dump.py --compare a.npz b.npz                          when gamd_amd._lib is imported)

The runs use the systems of tests/test_gpu_report.py (_Case).  The reporter, the recorder and the structure sampler are armed
together with the co-prime intervals 2, 3 and 5, so single, double and triple samples of one step all occur; the recorder
keeps 8 frames of 20, so frames are dropped as well.
  a  LJ, 258 atoms, BAOAB in skin mode, two md_run calls of 30 steps
  b  the same under the Nose-Hoover chain
  c  64 rigid TIP3P molecules with species, exclude_same_molecule, BAOAB
  d  two LJ boxes whose edge buffer is too small: the run freezes on the device and gamd_sync_status resumes it
Written per case: final x, v, f and every attribute of report_read(), traj_read() and structure_read().
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

STEPS = 30


def _arm(eng, case):
    water = case.kind == "water"
    eng.report_configure(2, rdf_bins=64, rdf_rmax=0.0 if water else 5.0, exclude_same_molecule=water, **case.report_kw())
    eng.traj_configure(3, max_frames=8, fields=("x", "v", "f", "image"), n_lags=4, subtract_com=True)
    eng.structure_configure(5, rdf_bins=64, sk_n2max=9, exclude_same_molecule=water)


def _collect(out, name, eng, x, v, f, extra=None):
    got = {"x": x.cpu().numpy(), "v": v.cpu().numpy(), "f": f.cpu().numpy(), **(extra or {})}
    for who, obj in (("report", eng.report_read()), ("traj", eng.traj_read()), ("structure", eng.structure_read())):
        got.update({f"{who}.{k}": val for k, val in vars(obj).items() if val is not None})
    out.update({f"{name}/{k}": np.asarray(val) for k, val in got.items()})
    eng.close()


def dump(path):
    from test_gpu_report import _Case
    from gamd_amd.engine import GamdForce
    out = {}
    for name, case in (("a", _Case("lj", skin=1.25)), ("b", _Case("lj", "nhc", skin=1.25)), ("c", _Case("water"))):
        eng, x, v, f = case.make()
        _arm(eng, case)
        chain = case.run(eng, x, v, f, STEPS)
        if name != "c":
            case.run(eng, x, v, f, STEPS, first_step=STEPS, chain=chain)
        _collect(out, name, eng, x, v, f)
    case = _Case("lj", n_boxes=2)
    big, x, v, f = case.make()                  # the start forces from an ample handle, as the overflow tests do
    big.close()
    eng = GamdForce(case.sd, case.n, case.box, case.rc, n_boxes=2, edge_capacity=4000, **case.eng_kw)
    _arm(eng, case)
    case.run(eng, x, v, f, STEPS, sync=False)
    _collect(out, "d", eng, x, v, f, {"resumed": eng.sync_status()})
    assert out["d/resumed"] == 1, "case d was meant to outgrow its edge buffer"
    np.savez(path, **out)
    print(f"{path}: {len(out)} entries from {os.environ.get('GAMD_LIB', 'the default library')}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()):
            bad.append(k)
    nonzero = sum(1 for k in a.files if a[k].size and np.any(a[k]))
    print(f"{len(a.files)} / {len(b.files)} entries ({nonzero} with a non-zero value), {len(bad)} differ" + "".join("\n  " + k for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
