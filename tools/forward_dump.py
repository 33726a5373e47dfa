#!/usr/bin/env python3
"""Everything the force evaluation and the MD driver hand back, for every kernel family, as one .npz — to set two builds of the
library against each other bit for bit — and, under a kernel trace, the launches of one force evaluation per family.

    GAMD_LIB=/path/to/libgamd_hip.so python tools/forward_dump.py out.npz        (one process per library: GAMD_LIB is read
    python tools/forward_dump.py --compare a.npz b.npz                            when gamd_amd._lib is imported)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/forward_dump.py --launches
    python tools/forward_dump.py --parse-trace DIR out.json                       (then compare the two .json files)

Dump: for every case of tests/lp_cases.py and the update-edge and selfloop cases of tests/test_weights_host.py, on the case's
system, normalised and denormalised forces through forward, forward_host and forward_edges (the edge list read back from
debug_edges); then x, v, f after 12 md_run steps of the systems of tests/test_gpu_report.py (_Case):
  skin / skin-com   LJ 258, BAOAB in skin mode, without and with remove_cm_motion
  exact             the same without a skin
  nhc               the Nose-Hoover chain
  water             64 rigid TIP3P molecules, BAOAB in skin mode (remove_cm_motion on)
  boxes2            two LJ boxes
  resume            two LJ boxes whose edge buffer is too small: the run freezes on the device and gamd_sync_status resumes it
--launches: per case and tile regime (the case's small_tile_limit; -1, the throughput kernels) one engine, a first evaluation,
then one between two marker kernels (a cumsum, which nothing else here launches); --parse-trace cuts the trace at the markers
and writes per "case/regime" the list of [kernel name with template arguments, grid size, workgroup size].
"""
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

STEPS = 12
EXTRA_IDS = ("update-edge", "selfloop")


def cases():
    """(id, case, seed, length, system, cutoff, flavour, edge dtype, kernel_select, small_tile_limit, self-loop mode) of every
    family: lp_cases.CASES, then the two EXTRA cases on water90."""
    import lp_cases as lc
    from test_weights_host import BY_ID
    out = [(c.id, c, c.seed, c.length, c.system, c.cutoff, c.flavour, c.edge_dtype, c.kernel_select, c.small_tile_limit, "dgl07_noop")
           for c in lc.CASES]
    for i in EXTRA_IDS:
        w = BY_ID[i]
        out.append((i, w, w.seed, w.length, "water90", 4.2, "jaxmd", w.edge_dtype, w.kernel_select, 0,
                    "append_zero_feature_loops" if w.self_loop else "dgl07_noop"))
    return out


def engine(case, small_tile_limit=None, **kw):
    import lp_cases as lc
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import make_state_dict
    cid, c, seed, length, system, cutoff, flavour, dtype, ksel, limit, loops = case
    pos, box, species, bonds = lc.system(system)
    eng = GamdForce(make_state_dict(c.cfg, seed, *length), pos.shape[0], box, cutoff, bond=bonds if c.cfg.use_bond else None,
                    nbr_flavour=flavour, cfg=c.cfg, edge_dtype=dtype, kernel_select=ksel, self_loop_mode=loops, scaler=(0.25, 2.0),
                    small_tile_limit=limit if small_tile_limit is None else small_tile_limit, **kw)
    return eng, torch.from_numpy(pos), species


def dump_forces(out):
    for case in cases():
        eng, pos, species = engine(case)
        for den in (False, True):
            tag = f"{case[0]}/{'denorm' if den else 'norm'}"
            out[tag + ".forward"] = eng.forward(pos, species=species, denormalize=den).cpu().numpy()
            out[tag + ".forward_host"] = eng.forward_host(pos.numpy(), species=species, denormalize=den).copy()
            edges = eng.debug_edges()
            out[tag + ".forward_edges"] = eng.forward_edges(pos, edges, species=species, denormalize=den).cpu().numpy()
        out[case[0] + "/counts"] = np.asarray(eng.counts()[:2])
        eng.close()


def dump_runs(out):
    from test_gpu_report import _Case
    from gamd_amd.engine import GamdForce
    runs = [("skin", _Case("lj", skin=1.25), {}), ("skin-com", _Case("lj", skin=1.25), {"remove_cm_motion": True}),
            ("exact", _Case("lj"), {}), ("nhc", _Case("lj", "nhc", skin=1.25), {}), ("water", _Case("water", skin=0.7), {}),
            ("boxes2", _Case("lj", n_boxes=2, skin=1.25), {})]
    for name, case, md in runs:
        eng, x, v, f = case.make()
        case.md.update(md)
        case.run(eng, x, v, f, STEPS)
        out.update({f"run-{name}/{k}": t.cpu().numpy() for k, t in (("x", x), ("v", v), ("f", f))})
        out[f"run-{name}/status"] = np.asarray(eng.last_status)
        eng.close()
    case = _Case("lj", n_boxes=2)
    big, x, v, f = case.make()                  # the start forces from an ample handle, as the overflow tests do
    big.close()
    eng = GamdForce(case.sd, case.n, case.box, case.rc, n_boxes=2, edge_capacity=4000, **case.eng_kw)
    case.run(eng, x, v, f, STEPS, sync=False)
    out["run-resume/resumed"] = np.asarray(eng.sync_status())
    assert out["run-resume/resumed"] == 1, "the resume run was meant to outgrow its edge buffer"
    out.update({f"run-resume/{k}": t.cpu().numpy() for k, t in (("x", x), ("v", v), ("f", f))})
    eng.close()


def dump(path):
    out = {}
    dump_forces(out)
    dump_runs(out)
    np.savez(path, **out)
    print(f"{path}: {len(out)} entries from {os.environ.get('GAMD_LIB', 'the default library')}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()):
            bad.append(k)
    nonzero = sum(1 for k in a.files if a[k].size and np.any(a[k]) and np.all(np.isfinite(a[k])))
    print(f"{len(a.files)} / {len(b.files)} entries ({nonzero} finite with a non-zero value), {len(bad)} differ" + "".join("\n  " + k for k in bad))
    return 1 if bad else 0


def launches():
    mark = torch.ones(3, device="cuda")
    for case in cases():
        for regime, limit in (("case", None), ("throughput", -1)):
            eng, pos, species = engine(case, small_tile_limit=limit)
            eng.forward(pos, species=species)
            mark.cumsum(0)
            eng.forward(pos, species=species)
            mark.cumsum(0)
            torch.cuda.synchronize()
            print(f"launches {case[0]}/{regime}", flush=True)
            eng.close()


def parse_trace(d, path):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def dims(r, what):
        return [int(r[k]) for k in sorted(r) if k.startswith(what)]
    keys = [f"{c[0]}/{regime}" for c in cases() for regime in ("case", "throughput")]
    cuts, inside, cur = [], False, []
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        if not name.startswith("k_") and ("cumsum" in name.lower() or "scan" in name.lower()):
            if inside:
                cuts.append(cur)
            inside, cur = not inside, []
        elif inside and name.startswith("k_"):
            cur.append([name.split("(")[0], dims(r, "Grid_Size"), dims(r, "Workgroup_Size")])
    assert len(cuts) == len(keys), f"{len(cuts)} marked evaluations in the trace, {len(keys)} expected"
    with open(path, "w") as f:
        json.dump(dict(zip(keys, cuts)), f, indent=0)
    print(f"{path}: {len(keys)} evaluations, {sum(map(len, cuts))} launches")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "--parse-trace":
        sys.exit(parse_trace(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 2 and sys.argv[1] == "--launches":
        sys.exit(launches())
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
