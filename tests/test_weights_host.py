"""Weight transformation and packing (gamd_amd/csrc/gamd_weights_host.h) without a GPU: tools/weights_host_check.cpp, built once
with the address and undefined-behaviour sanitizers, packs the seeded weights of every kernel family, and the sha256 of the blob
and of the printed offset / flag / scalar table must equal tests/golden/weight_blob_digests.json, which was recorded from the
library before packing left gamd_finalize_weights (the fixture names that commit).  The fixture also holds the sha256 of each
case's input tensors, so that a torch whose seeded draws differ is reported as that and not as a packing difference.

Cases: every entry of lp_cases.CASES as tests/test_gpu_lp_stages.py creates its engine (keep_stages=True), plus EXTRA below.
Which case reaches which branch of the packing path:
  update_edge override, per-layer edge_layer_norm, e_ln_* offsets   update-edge (128 wide: wide_enc / wide_conv / ln_fold overridden),
                                                                     update-edge-odd (zero-padded)
  update_edge refusals, missing key, wrong shape                     test_refusals_come_back_with_their_codes_and_texts
  zero padding in get()                                              wide-odd, f32-wide-odd, f16x3-wide-odd, f32-water-d256, lj-narrow
  BatchNorm fold                                                     bn, f32-bn, f32-bn5, f16x3-bn5, bf16-lj-bn5, fold-lj-bn
  log2 e / ln 2 rescaling, F2 order of W4 / b4 (bf16, 128 wide)      lj-1, lj-3, water-bond, bn, sparse, tiny, bf16-lj-bn5
  layer-0 form: LayerNorm hn0 / BatchNorm hn0                        f32-lj-3, f32-lj-1, fold-lj, lj-narrow / f32-bn, f32-bn5, fold-lj-bn
  layer-0 form off under kernel_select 4                             f32-lj-3-nohoist
  edge images: bf16 128 / split-fp16 128                             lj-1 ... tiny / ctl-f16x3 ... f16x3-tiny
  edge images: bf16 wide / split-fp16 wide                           wide-256, wide-odd, dynbox-noexp(-s27) / f16x3-wide-256, -odd, -dynbox-noexp
  edge images: fp32 folded W1 (A, a, b1')                            fold-water, fold-lj, fold-lj-bn, lj-narrow
  edge images: fp32 plain W1, F2-ordered W4                          ctl-f32, f32-water-bond, f32-lj-3, selfloop, fold-water-ks8, fold-lj-ks8
  edge images: fp32 generic width + the wide16.hip image             f32-wide-256(-tp, -hq), f32-wide-odd, f32-dynbox-noexp, f32-generic-128
  edge images: hidden_dim above 128 (DT = 2), encoder first Linear   f32-lj-d192, f32-water-d256
  node matrices: pack16 / pack16 split-fp16 / blocks / blocks f16    ctl-f32 / ctl-f16x3, lj-1 / f32-wide-256 / wide-256, f16x3-wide-256
  encoder first Linear: fp32 / bf16 / split-fp16, 44 / 45 / 4 feat.  ctl-f32 / lj-1 / ctl-f16x3, water-bond, f32-dynbox-noexp
  encoder W2, W3: generic width in split-fp16 (enc_wide_f16)         wide-256, f16x3-wide-256
  centred last encoder Linear / left alone (bf16, f16x3 128)         every fp32 and generic-width case / lj-1, ctl-f16x3
  folded encoder (R, Q^T c)                                          fold-water, fold-lj, fold-lj-bn, lj-narrow
  no RBF expansion (64 zero floats for the centres)                  dynbox-noexp, f32-dynbox-noexp, f16x3-dynbox-noexp
  uniform RBF grid found / not found                                 every expanded case / edited-centres
  node_emb (LJ) / node_encoder (water)                               lj-1 / ctl-f32
  appended self loops (fold off)                                     selfloop
"""
import hashlib
import json
import os
import shutil
import struct
import subprocess
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import pytest

import lp_cases
from gamd_amd.weights import ModelConfig, make_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "weight_blob_digests.json")
KIND = {"lj": 0, "water": 1, "dynbox": 1}
DTYPE = {"f32": 0, "bf16": 1, "f16x3": 2}


@dataclass(frozen=True)
class WCase:
    id: str
    cfg: ModelConfig
    seed: int
    length: tuple
    edge_dtype: str = "f32"
    kernel_select: int = 0
    keep_stages: bool = False
    self_loop: int = 0
    edit: Optional[str] = None         # "centres": one RBF centre moved off the grid


_W, _LJ = lp_cases._w, lp_cases._lj
EXTRA = [
    WCase("fold-water", _W(), 29, (2.9, 1.1)),
    WCase("fold-lj", _LJ(3), 22, (5.0, 1.7)),
    WCase("fold-lj-bn", _LJ(2, use_layer_norm=False), 24, (5.0, 1.7)),
    WCase("fold-water-ks8", _W(), 29, (2.9, 1.1), kernel_select=8),
    WCase("fold-lj-ks8", _LJ(3), 22, (5.0, 1.7), kernel_select=8),
    WCase("lj-narrow", _LJ(2, encoding_size=100, hidden_dim=72, edge_embedding_dim=90), 36, (5.0, 1.7)),
    WCase("selfloop", _W(), 29, (2.9, 1.1), self_loop=1),
    WCase("update-edge", ModelConfig(kind="dynbox", conv_layer=2, update_edge=True), 34, (2.9, 1.1)),
    WCase("update-edge-odd", ModelConfig(kind="dynbox", conv_layer=2, update_edge=True, encoding_size=96, hidden_dim=64,
                                         edge_embedding_dim=96), 35, (2.9, 1.1)),
    WCase("bf16-lj-bn5", _LJ(5, use_layer_norm=False), 31, (5.0, 1.7), edge_dtype="bf16"),
    WCase("edited-centres", _W(), 29, (2.9, 1.1), edit="centres"),
]
CASES = [WCase(c.id, c.cfg, c.seed, c.length, c.edge_dtype, c.kernel_select, True) for c in lp_cases.CASES] + EXTRA
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ARITH_IDS = ["f32-bn", "lj-narrow", "ctl-f32", "f32-wide-odd", "f32-water-d256", "update-edge-odd"]


def state_dict(c: WCase):
    sd = make_state_dict(c.cfg, c.seed, *c.length)
    if c.edit == "centres":
        sd["edge_expand.centers"][7] += 1e-3
    return sd


def tensors(c: WCase):
    """[(name, float32 array)] as GamdForce hands them to gamd_load_weight."""
    return [(k, np.ascontiguousarray(v.numpy().astype(np.float32))) for k, v in state_dict(c).items() if not k.endswith("num_batches_tracked")]


def input_digest(ts) -> str:
    h = hashlib.sha256()
    for _, a in ts:
        h.update(a.tobytes())
    return h.hexdigest()


def spec(c: WCase):
    """The 16 fields of WeightSpec: gamd_config's and the three flags gamd_create decides from it."""
    g = c.cfg
    Ht, Et, Dt = g.encoding_size, g.edge_embedding_dim, g.hidden_dim
    H, Eh, Dp = (128 if Ht <= 128 else 256), (128 if Et <= 128 else 256), (128 if Dt <= 128 else 256)
    f32, no_expand = c.edge_dtype == "f32", g.n_rbf == 0
    generic = H != 128 or Eh != 128 or no_expand
    forced = bool(c.kernel_select & 1) and f32
    lp_generic = not f32 and (generic or (Ht, Et, Dt) != (128, 128, 128))
    wide_enc = generic or forced or lp_generic or Dp > 128
    wide_conv = H != 128 or Eh != 128 or forced or lp_generic or Dp > 128
    ln_fold = f32 and not wide_enc and not wide_conv and c.self_loop == 0 and not c.keep_stages and not c.kernel_select & 8
    return [KIND[g.kind], DTYPE[c.edge_dtype], int(no_expand), c.self_loop, c.kernel_select, g.conv_layer,
            (4 if no_expand else 44) + int(g.use_bond), Ht, Et, Dt, H, Eh, Dp, int(wide_enc), int(wide_conv), int(ln_fold)]


def write_case(path, fields, ts):
    with open(path, "wb") as f:
        f.write(struct.pack("<16i", *fields))
        f.write(struct.pack("<i", len(ts)))
        for name, a in ts:
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<i", a.ndim) + struct.pack(f"<{a.ndim}q", *a.shape))
            f.write(a.astype("<f4").tobytes())


def host_compiler() -> str:
    """ROCm's clang++, next to hipcc: it knows _Float16 (the system g++ may not) and links the sanitizer runtimes into the program."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    tried = []
    for base in (os.path.dirname(os.path.realpath(hipcc)), os.path.dirname(hipcc)):
        for rel in ("../llvm/bin/clang++", "../lib/llvm/bin/clang++", "clang++"):
            cand = os.path.normpath(os.path.join(base, rel))
            tried.append(cand)
            if os.access(cand, os.X_OK):
                return cand
    raise AssertionError("tools/weights_host_check.cpp needs ROCm's clang++ (for _Float16); looked for " + ", ".join(tried))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("weights_host") / "weights_host_check"
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "weights_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def test_header_is_plain_cxx_without_a_rocm_include_path(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "gamd_weights_host.h"\nint main() { return 0; }\n')
    run = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "gamd_amd", "csrc"), str(src)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(BY_ID)


@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_packed_image_is_what_the_fixture_recorded(case_id, check_exe, golden, tmp_path):
    c = BY_ID[case_id]
    ts = tensors(c)
    want = golden[case_id]
    assert input_digest(ts) == want["inputs"], "the seeded weights differ from the ones the fixture was recorded with"
    write_case(tmp_path / "case.bin", spec(c), ts)
    run = subprocess.run([check_exe, "pack", str(tmp_path / "case.bin"), str(tmp_path / "blob.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert not run.stdout.startswith("error"), run.stdout
    table = hashlib.sha256(run.stdout.encode()).hexdigest()
    blob = hashlib.sha256((tmp_path / "blob.bin").read_bytes()).hexdigest()
    assert table == want["table"], "offset / flag / scalar table differs:\n" + run.stdout
    assert blob == want["blob"], "the packed blob differs"


@pytest.mark.parametrize("case_id", ARITH_IDS)
def test_host_arithmetic_against_a_naive_restatement(case_id, check_exe, tmp_path):
    c = BY_ID[case_id]
    write_case(tmp_path / "case.bin", spec(c), tensors(c))
    run = subprocess.run([check_exe, "arith", str(tmp_path / "case.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.rstrip().endswith("arith: ok"), run.stdout + run.stderr
    expected = {"f32-bn": ("BatchNorm alpha / beta", "M0 and c0"), "lj-narrow": ("M0 and c0",), "ctl-f32": ("centred W_e3",),
                "f32-wide-odd": ("centred W_e3", "padded rows and columns of every"), "f32-water-d256": ("padded rows and columns of every",),
                "update-edge-odd": ("padded rows and columns of every",)}[case_id]
    for line in ("permute_f2 is the permutation",) + expected:
        assert "arith: " + line in run.stdout, run.stdout


def test_refusals_come_back_with_their_codes_and_texts(check_exe, tmp_path):
    def refusal(c, ts, fields=None):
        write_case(tmp_path / "case.bin", fields or spec(c), ts)
        run = subprocess.run([check_exe, "pack", str(tmp_path / "case.bin"), str(tmp_path / "blob.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
        return run.stdout.rstrip("\n")

    c = BY_ID["ctl-f32"]
    ts = tensors(c)
    assert refusal(c, [t for t in ts if t[0] != "graph_decoder.mlp_layer.2.bias"]) == "error -2 missing weight 'graph_decoder.mlp_layer.2.bias'"
    # a wrong shape carries its own text; the code that reaches the caller has always been the -2 of the group it was looked up in
    bad = [(k, np.zeros(2, np.float32) if k == "length_std" else a) for k, a in ts]
    assert refusal(c, bad) == "error -2 weight 'length_std' has shape (2,), expected (1,) for this configuration"
    u = BY_ID["update-edge"]
    uneven = replace(u, cfg=replace(u.cfg, edge_embedding_dim=96))
    assert refusal(uneven, tensors(uneven)) == "error -22 update_edge_emb needs encoding_size == edge_embedding_dim (got 128, 96)"
    lowp = replace(u, edge_dtype="bf16")
    assert refusal(lowp, tensors(lowp)) == "error -22 update_edge_emb is built for the fp32 edge MLP without appended self loops"
