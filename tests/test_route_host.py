"""The kernel route (gamd_amd/csrc/gamd_route_host.h) without a GPU: tools/route_host_check.cpp, built once with the address and
undefined-behaviour sanitizers, prints the route of every case of tests/test_weights_host.py (lp_cases.CASES and EXTRA) for an
edge estimate of one tile and for one above small_tile_limit, and the flags, widths, enumerators, small_tiles and the kernel
names of one force evaluation must be what tests/golden/forward_routes.json holds.  The fixture was recorded from the library
before the route had a header of its own (its note says from which lines and which trace), so a route that reaches another kernel
than the one whose weights pack_weights laid out fails here.  The refusals that moved into the header come back by code and text."""
import json
import os
import subprocess

import pytest

import lp_cases
from test_weights_host import BY_ID, CASES, DTYPE, KIND, ROOT, host_compiler

FIXTURE = os.path.join(ROOT, "tests", "golden", "forward_routes.json")
DEFAULT_LIMIT = 512          # gamd_config.small_tile_limit = 0


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route_host") / "route_host_check"
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "route_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def tile_limit(c) -> int:
    """gamd_config.small_tile_limit of the case: lp_cases' own, 0 (the default) for the EXTRA cases."""
    return lp_cases.BY_ID[c.id].small_tile_limit if c.id in lp_cases.BY_ID else 0


def config(c):
    """The ten fields of RouteConfig (gamd_config's, from which the route follows) and n_layers."""
    g = c.cfg
    return [KIND[g.kind], DTYPE[c.edge_dtype], g.encoding_size, g.edge_embedding_dim, g.hidden_dim, int(g.n_rbf == 0), int(g.use_bond),
            c.self_loop, int(c.keep_stages), c.kernel_select, g.conv_layer]


def route(exe, fields, update_edge, limit, e_est):
    """The check program's output as {first word: rest of the line}; fields: as `config` gives them."""
    args = [*fields[:10], int(update_edge), fields[10], limit, e_est]
    run = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    return dict(line.split(" ", 1) for line in run.stdout.splitlines())


def pairs(text):
    return {k: int(v) if v.lstrip("-").isdigit() else v for k, v in (item.split("=") for item in text.split())}


def test_header_is_plain_cxx_without_a_rocm_include_path(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "gamd_route_host.h"\nint main() { return 0; }\n')
    run = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "gamd_amd", "csrc"), str(src)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(BY_ID)


@pytest.mark.parametrize("estimate", ["one_tile", "above_limit"])
@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_route_is_what_the_fixture_recorded(case_id, estimate, check_exe, golden):
    c, want = BY_ID[case_id], golden[case_id]
    limit = tile_limit(c)
    held = DEFAULT_LIMIT if limit == 0 else limit
    e_est = 32 if estimate == "one_tile" else 32 * (max(held, 0) + 1) + 32
    got = route(check_exe, config(c), c.cfg.update_edge, limit, e_est)
    assert "error" not in got, got
    assert pairs(got["flags"]) == want["flags"]
    assert pairs(got["widths"]) == want["widths"]
    assert pairs(got["route"]) == want["route"]
    assert int(got["small_tiles"]) == want[estimate]["small_tiles"]
    assert got["kernels"].split() == want[estimate]["kernels"]


def test_both_tile_regimes_are_met(golden):
    """The two estimates reach different kernels exactly where the family has a small-tile kernel and the case lets it run."""
    differ = {i for i, w in golden.items() if w["one_tile"]["kernels"] != w["above_limit"]["kernels"]}
    assert {"ctl-f32", "f32-lj-3", "f32-wide-256", "update-edge", "fold-lj"} <= differ
    assert not differ & {"f32-tiny-tp", "f32-wide-256-tp", "f32-wide-256-hq", "f32-lj-d192", "lj-1", "ctl-f16x3", "wide-256"}
    assert all(w["above_limit"]["small_tiles"] == 0 for w in golden.values())


def test_refusals_come_back_with_their_codes_and_texts(check_exe):
    def refusal(update_edge=False, **kw):
        f = dict(kind=KIND["water"], dtype=DTYPE["f32"], enc=128, edge=128, hidden=128, no_expand=0, bond=0, loops=0, keep=0, ksel=0, layers=2)
        f.update(kw)
        got = route(check_exe, list(f.values()), update_edge, 0, 32)
        assert list(got) == ["error"], got
        return got["error"]

    assert refusal(enc=257) == "-22 encoding_size and edge_embedding_dim must be in [1, 256] (got 257, 128)"
    assert refusal(edge=-1) == "-22 encoding_size and edge_embedding_dim must be in [1, 256] (got 128, -1)"
    assert refusal(hidden=300) == "-22 hidden_dim must be in [1, 256] (got 300)"
    assert refusal(hidden=192, dtype=DTYPE["bf16"]) == "-22 hidden_dim above 128 is built for edge_dtype f32 only (got hidden_dim 192)"
    assert refusal(hidden=256, dtype=DTYPE["f16x3"]) == "-22 hidden_dim above 128 is built for edge_dtype f32 only (got hidden_dim 256)"
    assert refusal(True, edge=96) == "-22 update_edge_emb needs encoding_size == edge_embedding_dim (got 128, 96)"
    assert refusal(True, dtype=DTYPE["bf16"]) == "-22 update_edge_emb is built for the fp32 edge MLP without appended self loops"
    assert refusal(True, loops=1) == "-22 update_edge_emb is built for the fp32 edge MLP without appended self loops"
    # the widths are judged before update_edge is, and 0 stands for 128
    assert refusal(True, enc=0, edge=300) == "-22 encoding_size and edge_embedding_dim must be in [1, 256] (got 128, 300)"
