"""No-GPU checks of the GEMM dispatcher: cst_gemm_route (csrc/gemm.hip: gemm_route) names, for a descriptor, the kernel cst_gemm
launches.  The expected routes were RECORDED from the dispatcher as it was before it became one route function (its launchers
patched to write the text instead of launching), so "the refactor changed no decision" is asserted row by row: the table below
(the launches of the training step, of decoding and of the pos-conv stack) and the denser grid in golden/gemm_route_grid.json
(both sides of every threshold in the code x layouts x dtypes x epilogue kinds x split_k x batching x row limits; rejected
descriptors are recorded with their code and message).  The operand addresses are fake: the query reads no memory.

A row is "M N K layout [flags] [key=value]": bf16 unless f32; leading dimensions K (k-major) or M / N (mn-major) and ldc = N unless
given; split_k = -1 unless split=; bias = BIAS_COL; act / dact = GELU; aux_out / aux_in / resid have leading dimension N."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_pkg

GRID = os.path.join(GOLDEN, "gemm_route_grid.json")
FLAGS = {"f32", "cf32", "bias", "biasrow", "act", "aux_out", "dact", "resid", "drop", "colsum", "m_len", "m_live", "k_live", "k_len"}
KEYS = {"split", "b0", "b1", "lda", "ldb", "ldc", "a_seg", "a_seg_stride", "b_seg", "b_seg_stride", "alpha"}
# the switches that left the dispatcher: setting them must change nothing
REMOVED = {"CST_GEMM_8P_ALL": "1", "CST_GEMM_FORCE_8P": "1", "CST_GEMM_NO_8P": "1", "CST_GEMM_8P_NO_DACT": "1", "CST_GEMM_GLDS_ALL": "1",
           "CST_GEMM_NO_GLDS": "1", "CST_GEMM_NO_MID8P": "1", "CST_GEMM_NO_SKINNY": "1", "CST_GEMM_SKINNY_NS4": "1",
           "CST_GEMM_SKINNY_TILES": "512", "CST_GEMM_NO_SPLIT_ORDER": "1", "CST_GEMM8P_CUS": "64", "CST_GEMM8P_NO_GPERM": "1",
           "CST_GEMM_4W_GROUP_M": "4"}

TABLE = [
    ("31760 768 3072 kk bias resid drop", "4w"),
    ("31760 768 768 kk bias resid drop", "8p kk"),
    ("31760 2304 768 kk bias", "8p kk"),
    ("31760 3072 768 kk bias act aux_out", "8p kk"),
    ("31760 3072 768 kk dact", "8p kk"),
    ("31760 768 3072 kk resid", "4w"),
    ("31760 768 3072 kk resid m_live", "4w"),
    ("47968 768 3072 kk bias resid", "4w"),
    ("40000 768 3072 kk bias resid", "8p kk"),
    ("24000 768 1536 kk", "4w"),
    ("31760 768 3072 kk bias act", "8p kk"),
    ("8000 768 3072 kk", "glds bf16 kk 128x128 nt256 ns2 split1"),
    ("31760 768 3072 km", "8p km"),
    ("31760 3072 768 km dact", "8p km"),
    ("24000 2560 512 km split=1", "8p km"),
    ("4064 512 10000 km", "8p km"),
    ("768 3072 31760 mm colsum", "reg bf16 mm 256x256 nt1024 split7"),
    ("3072 768 31760 mm colsum k_live", "reg bf16 mm 256x256 nt1024 split7"),
    ("768 768 31760 mm colsum", "reg bf16 mm 256x256 nt1024 split28"),
    ("2304 768 31760 mm", "reg bf16 mm 256x256 nt1024 split9"),
    ("10000 512 4064 mm", "reg bf16 mm 256x256 nt1024 split3"),
    ("512 512 7901 mm colsum", "reg bf16 mm 128x128 nt256 colsum split15"),
    ("1536 512 7901 mm", "reg bf16 mm 128x128 nt256 split5"),
    ("512 2048 7901 mm colsum", "reg bf16 mm 128x128 nt256 colsum split4"),
    ("2048 512 7901 mm colsum", "reg bf16 mm 128x128 nt256 colsum split4"),
    ("512 512 64 mm", "reg bf16 mm 128x128 nt256 split1"),
    ("64 264 4096 mm", "reg bf16 mm 64x128 nt256 split8"),
    ("72 6144 4096 mm", "reg bf16 mm 128x128 nt256 split5"),
    ("2048 2048 4096 mk", "reg bf16 mk 256x256 nt1024 split4"),
    ("7901 512 512 kk bias", "glds bf16 kk 64x64 nt256 ns2 split1"),
    ("7901 512 2048 kk bias resid", "glds bf16 kk 64x64 nt256 ns2 split1"),
    ("7901 2048 512 kk bias act aux_out", "8p kk"),
    ("7901 1536 512 kk bias", "8p kk"),
    ("7901 1536 512 kk dact resid", "glds bf16 kk 128x128 nt256 ns2 split1"),
    ("4064 1536 512 kk bias", "glds bf16 kk 128x128 nt256 ns2 split1"),
    ("12000 512 512 kk", "glds bf16 kk 128x128 nt256 ns2 split1"),
    ("4064 10000 512 kk", "8p kk"),
    ("160 512 512 kk bias", "glds bf16 kk 64x64 nt256 ns4 split1"),
    ("160 10000 512 kk", "glds bf16 kk 64x64 nt256 ns4 split1"),
    ("256 2048 512 kk", "glds bf16 kk 64x64 nt256 ns4 split1"),
    ("257 64 768 kk", "glds bf16 kk 128x64 nt256 ns2 split1"),
    ("31760 64 768 kk f32", "glds f32 kk 128x64 nt256 ns2 split1"),
    ("1499 48 6144 kk b0=32 b1=16 lda=48 ldc=768 bias act aux_out resid split=1 m_len", "glds bf16 kk 128x64 nt256 ns2 split1"),
    ("48 6144 50000 mm b1=16 lda=48 ldb=48 cf32 split=1 colsum k_live", "reg bf16 mm 64x128 nt256 colsum split1"),
    ("14999 512 1536 kk b0=32 lda=1024 act aux_out split=1 m_len", "8p kk"),
    ("14999 512 1024 kk b0=32 lda=512 ldc=1024 dact split=1 m_len", "8p kk"),
    ("512 1536 14999 mm b0=32 lda=512 ldb=1024 cf32 split=1 k_len", "reg bf16 mm 256x256 nt1024 split1"),
    ("512 1536 14999 mm b0=32 lda=512 ldb=1024 cf32 split=2 k_len", "reg bf16 mm 256x256 nt1024 split2"),
    ("4096 512 1024 kk a_seg=64 a_seg_stride=256", "reg bf16 kk seg 128x128 nt256 split2"),
    ("31760 768 768 kk f32 bias", "glds f32 kk 256x256 nt1024 ns2 split1"),
    ("1000 768 512 kk f32", "glds f32 kk 128x128 nt256 ns2 split2"),
    ("768 768 31760 mm f32 colsum", "reg f32 mm 256x256 nt1024 split28"),
    ("31760 768 3072 km f32", "reg f32 km 256x256 nt1024 split1"),
]


def parse(spec):
    t = spec.split()
    M, N, K = (int(x) for x in t[:3])
    lay, flags, kv = t[3], set(), {}
    assert lay in ("kk", "km", "mk", "mm"), spec
    for w in t[4:]:
        if "=" in w:
            k, v = w.split("=")
            assert k in KEYS, spec
            kv[k] = float(v) if k == "alpha" else int(v)
        else:
            assert w in FLAGS, spec
            flags.add(w)
    return M, N, K, lay, flags, kv


def make_desc(L, spec):
    """The descriptor of a row.  Every pointer is a fake, 16-byte-aligned address; the workspace is 'large enough'."""
    M, N, K, lay, flags, kv = parse(spec)
    addr = iter(range(1 << 32, 1 << 40, 1 << 32))
    d = L.GemmDesc()
    d.dtype = L.F32 if "f32" in flags else L.BF16
    d.c_dtype = L.F32 if "cf32" in flags else d.dtype
    d.a_kmajor, d.b_kmajor = int(lay[0] == "k"), int(lay[1] == "k")
    d.M, d.N, d.K = M, N, K
    d.A, d.B, d.C = next(addr), next(addr), next(addr)
    d.lda = kv.get("lda", K if d.a_kmajor else M)
    d.ldb = kv.get("ldb", K if d.b_kmajor else N)
    d.ldc = kv.get("ldc", N)
    d.a_seg, d.a_seg_stride = kv.get("a_seg", 0), kv.get("a_seg_stride", 0)
    d.b_seg, d.b_seg_stride = kv.get("b_seg", 0), kv.get("b_seg_stride", 0)
    if "bias" in flags or "biasrow" in flags:
        d.bias, d.bias_mode = next(addr), (L.BIAS_ROW if "biasrow" in flags else L.BIAS_COL)
    if "act" in flags:
        d.act = L.ACT_GELU
    if "aux_out" in flags:
        d.aux_out, d.ld_aux_out = next(addr), N
    if "dact" in flags:
        d.dact, d.aux_in, d.ld_aux_in = L.ACT_GELU, next(addr), N
    if "resid" in flags:
        d.resid, d.ld_resid = next(addr), N
    d.alpha = kv.get("alpha", 1.0)
    if "drop" in flags:
        d.drop_p, d.drop_key = 0.1, 1
    d.batch0, d.batch1 = kv.get("b0", 1), kv.get("b1", 1)
    if d.batch1 > 1:
        d.sa1, d.sb1, d.sc1 = M * K, N * K, M * N
    if d.batch0 > 1:
        d.sa0, d.sb0, d.sc0 = d.batch1 * M * K, d.batch1 * N * K, d.batch1 * M * N
    d.split_k = kv.get("split", -1)
    d.workspace, d.workspace_bytes = next(addr), 1 << 60
    for f in ("k_live", "m_live", "k_len", "m_len", "colsum"):
        if f in flags:
            setattr(d, f, next(addr))
    d.k_epoch = d.m_epoch = 1
    return d


def route_of(L, lib, spec):
    """The route text, or '!<code> <message>' for a descriptor cst_gemm rejects."""
    d = make_desc(L, spec)
    out = ctypes.create_string_buffer(128)
    rc = lib.cst_gemm_route(ctypes.byref(d), out, len(out))
    return out.value.decode() if rc == 0 else "!%d %s" % (rc, lib.cst_last_error().decode())


def grid_rows(full=False):
    """(row, route) of the recorded grid; full: (row, route, cst_gemm_splits, cst_gemm_colsum_is_fused, cst_gemm_workspace) as the
    dispatcher answered before (those three validate nothing, so rejected rows have them too)."""
    with open(GRID) as f:
        return [tuple(r) if full else tuple(r[:2]) for r in json.load(f)["rows"]]


def mismatches(L, lib, rows):
    return [(spec, want, got) for spec, want in rows for got in [route_of(L, lib, spec)] if got != want]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    L = load_pkg().lib
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    return L, L.load()


def test_the_table_of_step_and_decode_launches_routes_as_recorded(built):
    bad = mismatches(*built, TABLE)
    assert not bad, "%d of %d rows differ, e.g. %s" % (len(bad), len(TABLE), bad[:5])


def test_the_grid_routes_as_recorded(built):
    rows = grid_rows()
    assert len(rows) >= 2000 and any(w.startswith("!") for _, w in rows)
    for head in ("reg ", "glds ", "8p ", "4w"):
        assert any(w.startswith(head) for _, w in rows), head
    bad = mismatches(*built, rows)
    assert not bad, "%d of %d rows differ, e.g. %s" % (len(bad), len(rows), bad[:5])


def test_the_other_queries_are_views_of_the_route(built):
    """cst_gemm_splits, cst_gemm_colsum_is_fused and cst_gemm_workspace: on every grid row the values recorded before the refactor;
    on every accepted row in agreement with the route text (the text of the persistent kernel carries no split count: there the
    query is taken at its word) — split s > 1 => s M N nb 4 bytes of slabs; a fused column sum adds s M nb 4 bytes of slice sums
    when K is split, a separate one the column sum's own workspace."""
    L, lib = built
    n = 0
    for spec, _, s, fused, need in grid_rows(full=True):
        d = make_desc(L, spec)
        got = (lib.cst_gemm_splits(ctypes.byref(d)), lib.cst_gemm_colsum_is_fused(ctypes.byref(d)), lib.cst_gemm_workspace(ctypes.byref(d)))
        assert got == (s, fused, need), spec
    for spec, want in TABLE + grid_rows():
        if want.startswith("!"):
            continue
        d = make_desc(L, spec)
        M, N, K, _, flags, _ = parse(spec)
        nb = d.batch0 * d.batch1
        s = lib.cst_gemm_splits(ctypes.byref(d))
        fused = " colsum" in want
        assert s == (1 if want == "4w" else s if want.startswith("8p") else int(want.rsplit("split", 1)[1])), spec
        assert lib.cst_gemm_colsum_is_fused(ctypes.byref(d)) == int(fused), spec
        need = s * M * N * nb * 4 if s > 1 else 0
        if fused:
            need += s * M * nb * 4 if s > 1 else 0
        elif "colsum" in flags:
            need += lib.cst_colsum_workspace(K, M)
        assert lib.cst_gemm_workspace(ctypes.byref(d)) == need, spec
        n += 1
    assert n >= 1500


def test_a_rejected_descriptor_gets_the_code_and_message_of_cst_gemm(built):
    L, lib = built
    for spec in ("31760 768 3070 kk", "768 768 31760 kk colsum", "768 3072 31760 mm colsum b0=2","31760 768 768 kk dact"):
        d = make_desc(L, spec)
        if spec.endswith("dact"):
            d.aux_in = None
        out = ctypes.create_string_buffer(128)
        rc = lib.cst_gemm_route(ctypes.byref(d), out, len(out))
        msg = lib.cst_last_error()
        assert rc == L.load().cst_gemm(ctypes.byref(d), None) == -1 and lib.cst_last_error() == msg and out.value == b"", spec
    d = make_desc(L, "768 768 31760 mm")
    d.workspace_bytes = 16
    assert lib.cst_gemm_route(ctypes.byref(d), ctypes.create_string_buffer(128), 128) == -3
    assert b"split_k=28 needs" in lib.cst_last_error()


def test_the_removed_switches_change_no_route():
    """Own process: the dispatcher reads its switches once."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, **REMOVED))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout + r.stderr)[-2000:]


if __name__ == "__main__":
    L = load_pkg().lib
    rows = TABLE + grid_rows()
    bad = mismatches(L, L.load(), rows)
    print("ok %d" % len(rows) if not bad else "differ: %s" % bad[:5])
    sys.exit(1 if bad else 0)
