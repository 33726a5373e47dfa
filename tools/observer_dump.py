#!/usr/bin/env python3
"""Everything the five run observers, the two classical force sources and the two minimisers hand back, for short runs, as one
.npz — to set two builds of the library against each other bit for bit.

    GAMD_LIB=/path/to/libgamd_hip.so python tools/observer_dump.py out.npz      (one process per library: GAMD_LIB is read
    python tools/observer_dump.py --compare a.npz b.npz                          when gamd_amd._lib is imported)

The runs use the systems of tests/test_gpu_report.py (_Case).  The reporter, the recorder and the structure sampler are armed
together with the co-prime intervals 2, 3 and 5, so single, double and triple samples of one step all occur; the recorder
keeps 8 frames of 20, so frames are dropped as well.  The observer with a potential of the handle's kind (classical_configure
on LJ, water_classical_configure on water; shifted and switched) samples at the interval 7 into a log of 3 rows, so it meets
each of the others and drops rows.
  a  LJ, 258 atoms, BAOAB in skin mode, two md_run calls of 30 steps; then classical_forces on the final positions, in bohr
  b  the same under the Nose-Hoover chain
  c  64 rigid TIP3P molecules with species, exclude_same_molecule, BAOAB
  d  two LJ boxes whose edge buffer is too small: the run freezes on the device and gamd_sync_status resumes it
  e  two boxes of 86 rigid TIP3P molecules (258 atoms: two row tiles, molecule 85 straddles the tile edge at atom 256) with
     different positions and edges, 16 steps, the water classical observer alone at the interval 3; then
     water_classical_forces on the final positions, in bohr
  f  LJ force source: 258 atoms on the workload's lattice (two row tiles, the second partial), shifted and switched, 12 driven
     steps with every frame recorded and the classical observer at the interval 5
  g  water force source, 3-site: e's two boxes, 12 driven rigid steps, every frame recorded, the observer at the interval 3
  h  the same with the M-site (m_site = 0.1, gamd_water_msite); then water_classical_forces on the final positions
  i  gamd_minimize: 258 atoms (the lj258_seed0 snapshot), and a two-box handle (the snapshot and the lattice, different edges):
     40 iterations towards a tolerance they do not reach, with check_every = 1 and 16
  j  gamd_water_minimize: 86 molecules in a box with three different edges, the same 40 iterations and check_every
  fc, gc, hc, i2c  f, g, h and i's two-box handle with the pairs over the cell table (cells=True); gp: gc with particle-mesh Ewald
     (16^3, order 6).  Each also dumps the cell table (nc, start, order) of every box as the last evaluation left it
Between them every kernel of classical.hip, drive.hip, minimize.hip, water_classical.hip, water_drive.hip, water_msite.hip,
water_minimize.hip, cell_table.hip, water_cells.hip and classical_cells.hip writes into the dump: a partial tile, a molecule across
a tile edge, more than one slice, two boxes, and a k-vector list longer than one box needs.
Written per case: final x, v, f and every attribute of report_read(), traj_read(), structure_read() and
classical_read(forces=True) / water_classical_read(forces=True); for a, e and h what the call outside the run returned; for i
and j x, f, x64 and the rows of every call, and the observer's f_cl behind the last.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

STEPS = 30


def _arm(eng, case):
    water = case.kind == "water"
    eng.report_configure(2, rdf_bins=64, rdf_rmax=0.0 if water else 5.0, exclude_same_molecule=water, **case.report_kw())
    eng.traj_configure(3, max_frames=8, fields=("x", "v", "f", "image"), n_lags=4, subtract_com=True)
    eng.structure_configure(5, rdf_bins=64, sk_n2max=9, exclude_same_molecule=water)
    if water:
        eng.water_classical_configure(7, max_samples=3, **_water_kw(case.box))
    else:
        eng.classical_configure(7, max_samples=3)        # the defaults: shifted, switched over the last sigma


def _water_kw(box, unit=1.0):
    r_cut = 0.48 * float(np.min(box))
    return dict(sigma_o=3.15075 * unit, r_cut=r_cut * unit, r_switch=(r_cut - 1.0) * unit, shift=True, alpha=4.0 / r_cut / unit,
                k_cut=8.0 * 4.0 / r_cut / unit)


def _fields(obj):
    """what a read call returned from the device (the parameters it repeats, a dict, are the host's own)"""
    return {k: val for k, val in vars(obj).items() if val is not None and not isinstance(val, dict)}


def _tables(eng):
    """the cell table of every box as the last evaluation left it"""
    read = eng.classical_cells_table if eng.cfg.kind == "lj" else eng.water_cells_table
    return {f"cells.box{b}.{k}": val for b in range(eng.n_boxes) for k, val in zip(("nc", "start", "order"), read(b))}


def _collect(out, name, eng, x, v, f, extra=None, observers=("report", "traj", "structure"), outside=None, cells=False):
    water = eng.cfg.kind != "lj"
    got = {"x": x.cpu().numpy(), "v": v.cpu().numpy(), "f": f.cpu().numpy(), **(extra or {})}
    reads = [(who, getattr(eng, who + "_read")()) for who in observers]
    reads.append(("water_classical", eng.water_classical_read(forces=True)) if water else ("classical", eng.classical_read(forces=True)))
    for who, obj in reads:
        got.update({f"{who}.{k}": val for k, val in _fields(obj).items()})
    if outside:                                          # behind the reads: the call leaves its forces where forces=True reads them
        got.update(outside(eng))
    if cells:
        got.update(_tables(eng))
    out.update({f"{name}/{k}": np.asarray(val) for k, val in got.items()})
    eng.close()


def _bohr():
    from gamd_amd import workloads as wl
    return wl.BOHR_PER_NM, float(np.float32(wl.BOHR_PER_NM)) / 10.0


def _lj_outside(case, x):
    def call(eng):
        length, unit = _bohr()
        eng.classical_configure(0, sigma=3.4 * unit, r_cut=10.2 * unit, r_switch=6.8 * unit)
        f, e, w, c = eng.classical_forces((x.double() * unit).float(), box=case.box * unit, length_per_nm=length)
        return {"eval.forces": f.cpu().numpy(), "eval.energy": e, "eval.virial": w, "eval.pairs": c}
    return call


def _two_water_boxes():
    """e's system: (case, engine, x, v, f, boxes, species)"""
    import gamd_oracle as orc
    from gamd_amd import workloads as wl
    from gamd_amd.engine import GamdForce
    from test_gpu_water_classical import _Water
    case = _Water(n_mol=86)
    L = float(case.box)
    boxes = np.array([[L, L, L], [L, 1.03 * L, 1.01 * L]], dtype=np.float32)
    other = wl.water_box(86, seed=7, jitter=0.0, wrap=False)[0]
    pairs, _ = orc.water_constraints(case.n, wl.TIP3P_R_OH, wl.TIP3P_R_HH)
    mm = np.where(case.species == 1, wl.MASS_O, wl.MASS_H).astype(np.float64).reshape(-1, 1)
    v1 = np.random.default_rng(16).normal(0, 1.0, (case.n, 3)) * 10.0 * np.sqrt(wl.KB * 300.0 / mm)
    v1 = orc.rattle_velocities(other, v1, (1.0 / mm).reshape(-1), pairs)
    species = np.tile(case.species, 2)
    eng = GamdForce(case.sd, case.n, L, case.rc, n_boxes=2, **case.eng_kw)       # the edges differ from the first call on
    x = torch.from_numpy(np.concatenate([case.pos, other])).float().cuda()
    v = torch.from_numpy(np.concatenate([case.v0, v1])).float().cuda()
    f = eng.forward(x, box=boxes, species=species, denormalize=True).clone()
    return case, eng, x, v, f, boxes, species


def _water_outside(x, species, boxes, **kw):
    def call(eng):
        length, unit = _bohr()
        eng.water_classical_configure(0, **_water_kw(boxes, unit), **kw)
        fo, rd = eng.water_classical_forces((x.double() * unit).float(), species, box=boxes * unit, length_per_nm=length)
        return {"eval.forces": fo.cpu().numpy(), **{f"eval.{k}": val for k, val in _fields(rd).items()}}
    return call


def _water_two_boxes(out):
    """case e"""
    case, eng, x, v, f, boxes, species = _two_water_boxes()
    eng.water_classical_configure(3, max_samples=3, **_water_kw(boxes))
    eng.md_run(x, v, f, 16, gamma_per_ps=25.0, seed=11, box=boxes, **{**case.md, "species": species})
    _collect(out, "e", eng, x, v, f, observers=(), outside=_water_outside(x, species, boxes))


DRIVEN = 12


def _lj_source(out, name, cells=False):
    """cases f and fc"""
    from test_gpu_classical_drive import _Lj258
    case = _Lj258()
    eng, x, v, f = case.make()
    eng.classical_configure(5, max_samples=3, cells=cells)      # the defaults: shifted, switched over the last sigma
    eng.md_force_source("classical")
    f = eng.classical_forces(x)[0].float().contiguous()
    eng.traj_configure(1, max_frames=DRIVEN, fields=("x", "v", "f"))
    case.run(eng, x, v, f, DRIVEN)
    _collect(out, name, eng, x, v, f, observers=("traj",), cells=cells)


def _water_source(out, name, **kw):
    """cases g and h, gc, hc and gp"""
    case, eng, x, v, f, boxes, species = _two_water_boxes()
    eng.water_classical_configure(3, max_samples=3, **_water_kw(boxes), **kw)
    eng.md_force_source("water_classical")
    f = eng.water_classical_forces(x, species, box=boxes)[0].float().contiguous()
    eng.traj_configure(1, max_frames=DRIVEN, fields=("x", "v", "f"))
    eng.md_run(x, v, f, DRIVEN, gamma_per_ps=25.0, seed=11, box=boxes, **{**case.md, "species": species})
    _collect(out, name, eng, x, v, f, observers=("traj",), outside=_water_outside(x, species, boxes, **kw) if kw else None,
             cells=kw.get("cells", False))


def _minimise_calls(out, name, eng, call, read, cells=False):
    """40 iterations towards a tolerance they do not reach, looked at after every one and after every 16"""
    for every in (1, 16):
        res, x = call(tolerance=1e-300, max_iter=40, check_every=every)
        got = {"x": x, "f": res.f, "x64": res.x64}
        out.update({f"{name}/every{every}.{k}": val.cpu().numpy() for k, val in got.items()})
        out[f"{name}/every{every}.rows"] = np.asarray(res.rows)
        out[f"{name}/every{every}.status"] = np.asarray(res.status)
    out[f"{name}/f_cl"] = np.asarray(read(forces=True).forces)
    if cells:
        out.update({f"{name}/{k}": np.asarray(val) for k, val in _tables(eng).items()})
    eng.close()


def _minimisers(out):
    """cases i, i2c and j"""
    from test_gpu_classical_drive import _seeded_engine
    from test_gpu_minimize import _golden_start, _lattice_start
    from test_gpu_water_minimize import EDGES, _start, _water_engine
    (xa, ba), (xb, bb) = _golden_start(), _lattice_start()
    two = np.concatenate([xa, xb]), np.array([[ba] * 3, [bb] * 3], dtype=np.float32), 2
    for name, x0, box, nb in (("i1", xa, None, 1), ("i2",) + two, ("i2c",) + two):
        eng = _seeded_engine(258, float(ba), n_boxes=nb)
        if name == "i2c":
            eng.classical_configure(0, cells=True)

        def call(x0=x0, box=box, eng=eng, **kw):
            x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).cuda()
            return eng.minimize(x, box=box, return_x64=True, **kw), x
        _minimise_calls(out, name, eng, call, eng.classical_read, cells=name == "i2c")
    x0, box, species = _start(86, edges=EDGES)
    eng = _water_engine(86, box, 0.48 * float(np.min(box)))

    def call(**kw):
        x = torch.from_numpy(x0).cuda()
        return eng.water_minimize(x, species, box=box, return_x64=True, **kw), x
    _minimise_calls(out, "j", eng, call, eng.water_classical_read)


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
        _collect(out, name, eng, x, v, f, outside=_lj_outside(case, x) if name == "a" else None)
    case = _Case("lj", n_boxes=2)
    big, x, v, f = case.make()                  # the start forces from an ample handle, as the overflow tests do
    big.close()
    eng = GamdForce(case.sd, case.n, case.box, case.rc, n_boxes=2, edge_capacity=4000, **case.eng_kw)
    _arm(eng, case)
    case.run(eng, x, v, f, STEPS, sync=False)
    _collect(out, "d", eng, x, v, f, {"resumed": eng.sync_status()})
    assert out["d/resumed"] == 1, "case d was meant to outgrow its edge buffer"
    _water_two_boxes(out)
    _lj_source(out, "f")
    _lj_source(out, "fc", cells=True)
    _water_source(out, "g")
    _water_source(out, "h", m_site=0.1)
    _water_source(out, "gc", cells=True)
    _water_source(out, "hc", m_site=0.1, cells=True)
    _water_source(out, "gp", cells=True, pme=(16, 16, 16))
    _minimisers(out)
    np.savez(path, **out)
    print(f"{path}: {len(out)} entries from {os.environ.get('GAMD_LIB', 'the default library')}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()):
            bad.append(k)
    nonzero = sum(1 for k in a.files if a[k].size and np.any(a[k]))
    zero = [k for k in sorted(a.files) if "classical." in k and not (a[k].size and np.any(a[k]))]
    print("all-zero or empty entries of the observers with a potential: " + (", ".join(zero) or "none"))
    print(f"{len(a.files)} / {len(b.files)} entries ({nonzero} with a non-zero value), {len(bad)} differ" + "".join("\n  " + k for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
