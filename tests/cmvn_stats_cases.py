"""Case list of the CMVN statistics tests (tests/test_cmvn_stats_cases.py on the CPU, tests/test_gpu_cmvn_stats*.py on the GPU), a
numpy restatement of AccCmvnStats (src/feat/cmvn.cc:30-62), and how tests/golden/cmvn_stats.npz was made.

Inputs are regenerated from seeds and not stored; the fixture holds only what the reference's own compute-cmvn-stats (built by
`make -C oracle/ref_build featbin`) wrote for them, a hash of every generated input (a drifting generator is noticed), and a few of
the reference's output bytes for the table writers.

"Exact" utterances: x ~ N(15, 3) as float32, weights ~ N(0.5, 0.5) as float32 with every fifth weight set to 0.  On these every
fp64 partial sum is exactly representable, so no order of summation changes a bit: write_golden asserts that the reference equals
the restatement (fp32 products, math.fsum per column) bit for bit for every stored element and refuses to write otherwise, and
the device is held to bit equality with the fixture.

  shapes   (frames, D) = (1,1) (2,3) (255,43) (257,40) (3000,40) (20001,43) (700,257) (64,1320): per utterance, unweighted and
           weighted; the weighted table also holds `inf7x3`, whose row 5 is all infinities under weight 0.  (0,40) is a device-only
           case (the reference's Matrix cannot hold it): all zeros.
  d40      (257,40) (3000,40) (33,40): S = 3; per speaker for SPK2UTT (two utterances it lists are missing, one speaker has none),
           and global (the float matrix), unweighted and weighted; the counts of the log line and the exit status.
  b33_<u>  for each of the longer utterances u = 3000x40, 20001x43, 700x257: S = 33 ragged, u at position 17 among 32 short ones of
           its width.  The fixture holds a hash of the reference's 33 matrices (the short ones are restated in the test); u's own
           matrix is the one of `shapes`.
  wide     5000 x 7 with |x| = 10^U(-6,6) and random signs, unweighted and weighted.  Sums round here: the reference and the device
           are each held to |v - fsum| <= n * 2^-53 * sum |t_i| (n rows summed, t_i the fp32 terms): the first-order bound of any
           fp64 summation order, with one unit of slack over (n - 1) u.
"""
import hashlib
import json
import math
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmvn_stats.npz")

SHAPES = [(1, 1), (2, 3), (255, 43), (257, 40), (3000, 40), (20001, 43), (700, 257), (64, 1320)]
EMPTY = (0, 40)
LONG = [(3000, 40), (20001, 43), (700, 257)]
D40 = [(257, 40), (3000, 40), (33, 40)]
SPK2UTT = [("spkA", ["u257x40", "gone1", "u3000x40"]), ("spkB", ["u33x40", "gone2"]), ("spkC", ["gone3"])]
WIDE = (5000, 7)
B33_AT = 17


def name_of(T, D):
    return f"u{T}x{D}"


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def exact_utt(name, T, D):
    """(x [T x D] float32, w [T] float32) of an exact utterance: a function of its name alone."""
    rng = np.random.default_rng(_seed(name))
    x = rng.normal(15.0, 3.0, (T, D)).astype(np.float32)
    w = rng.normal(0.5, 0.5, T).astype(np.float32)
    w[::5] = 0.0
    return x, w


def utt(T, D):
    return exact_utt(name_of(T, D), T, D)


def inf_utt():
    x, w = exact_utt("inf7x3", 7, 3)
    x[5, :] = np.inf
    assert w[5] == 0.0
    return x, w


def wide_utt():
    rng = np.random.default_rng(_seed("wide"))
    T, D = WIDE
    x = (10.0 ** rng.uniform(-6.0, 6.0, (T, D)) * rng.choice([-1.0, 1.0], (T, D))).astype(np.float32)
    w = rng.normal(0.5, 0.5, T).astype(np.float32)
    w[::5] = 0.0
    return x, w


def b33(T, D):
    """The batch of 33 around the long utterance (T, D): [(name, x, w)], the long one at B33_AT."""
    out = []
    for i in range(33):
        if i == B33_AT:
            out.append((name_of(T, D),) + utt(T, D))
        else:
            t = 1 + (7 * i * i + 3 * i) % 300
            n = f"f{i:02d}_{t}x{D}"
            out.append((n,) + exact_utt(n, t, D))
    return out


def terms(x, w=None):
    """The fp32 terms the reference adds, rows of weight 0 left out: (x * w, (x * x) * w, w) as float32."""
    x = np.asarray(x, np.float32)
    if w is None:
        return x, x * x, np.ones(x.shape[0], np.float32)
    w = np.asarray(w, np.float32)
    keep = w != 0
    xs, ws = x[keep], w[keep][:, None]
    with np.errstate(all="ignore"):
        return xs * ws, (xs * xs) * ws, w[keep]


def restate(x, w=None):
    """AccCmvnStats: [2 x (D+1)] float64, every sum exactly rounded (math.fsum) over the fp32 terms."""
    t1, t2, ws = terms(x, w)
    D = np.asarray(x).shape[1]
    out = np.zeros((2, D + 1), np.float64)
    for d in range(D):
        out[0, d] = math.fsum(t1[:, d].astype(np.float64))
        out[1, d] = math.fsum(t2[:, d].astype(np.float64))
    out[0, D] = math.fsum(ws.astype(np.float64))
    return out


def order_bound(x, w=None):
    """n * 2^-53 * sum |t_i| per element of the statistics matrix (the count's terms are the weights)."""
    t1, t2, ws = terms(x, w)
    D = np.asarray(x).shape[1]
    n = t1.shape[0]
    out = np.zeros((2, D + 1), np.float64)
    out[0, :D] = np.abs(t1.astype(np.float64)).sum(axis=0)
    out[1, :D] = np.abs(t2.astype(np.float64)).sum(axis=0)
    out[0, D] = np.abs(ws.astype(np.float64)).sum()
    return out * (n * 2.0 ** -53) * (1 + 2.0 ** -40)     # (the bound's own sum rounds)


def input_hash(x, w):
    return hashlib.sha256(np.ascontiguousarray(x, np.float32).tobytes() + np.ascontiguousarray(w, np.float32).tobytes()).hexdigest()[:16]


def all_inputs():
    """name -> (x, w) of every generated input."""
    out = {name_of(T, D): utt(T, D) for T, D in SHAPES + D40}
    out["inf7x3"] = inf_utt()
    out["wide"] = wide_utt()
    for T, D in LONG:
        for n, x, w in b33(T, D):
            out[n] = (x, w)
    return out


def matrices_hash(mats):
    return hashlib.sha256(b"".join(np.ascontiguousarray(m, "<f8").tobytes() for m in mats)).hexdigest()


def load():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------- how the fixture was made
def fv_entry(key, w):
    """`key ` + Vector<float>::Write in binary (src/cpucompute/vector.cc): what --weights=ark:... reads."""
    return key.encode() + b" \x00BFV \x04" + struct.pack("<i", len(w)) + np.ascontiguousarray(w, "<f4").tobytes()


def spk2utt_text():
    return "".join(f"{s} {' '.join(u)}\n" for s, u in SPK2UTT)


def write_golden(bindir, path=GOLDEN):
    """Runs the reference's compute-cmvn-stats (in `bindir`) on binary archives of every case and stores its outputs."""
    from eesen_amd import kaldi_io
    tool = os.path.join(bindir, "compute-cmvn-stats")
    data = {"hashes": json.dumps({n: input_hash(x, w) for n, (x, w) in sorted(all_inputs().items())})}

    def run(tmp, tag, items, weighted, extra=(), out=None):
        """items: [(name, x, w)] -> (returncode, stderr, output path)"""
        feats, wark = os.path.join(tmp, tag + ".ark"), os.path.join(tmp, tag + "_w.ark")
        kaldi_io.write_mat_ark(feats, [(n, x) for n, x, _ in items])
        with open(wark, "wb") as f:
            for n, _, w in items:
                f.write(fv_entry(n, w))
        out = out or "ark:" + os.path.join(tmp, tag + "_out.ark")
        r = subprocess.run([tool] + list(extra) + (["--weights=ark:" + wark] if weighted else []) + ["ark:" + feats, out], capture_output=True, text=True)
        return r, out.split(":", 1)[-1]

    def exact(got, x, w, what):
        want = restate(x, w)
        assert got.shape == want.shape and np.array_equal(got, want), f"{what}: the reference differs from the exact sums: not an exact case"

    def counts(r):
        m = re.search(r"Done accumulating CMVN stats for (\d+) utterances; (\d+) had errors", r.stderr)
        assert m, r.stderr
        return [int(m.group(1)), int(m.group(2)), r.returncode]

    with tempfile.TemporaryDirectory() as tmp:
        # shapes: per utterance
        for weighted in (False, True):
            tag = "w" if weighted else "u"
            items = [(name_of(T, D),) + utt(T, D) for T, D in SHAPES] + ([("inf7x3",) + inf_utt()] if weighted else [])
            r, out = run(tmp, "shapes_" + tag, items, weighted)
            got = dict(kaldi_io.read_mat64_table("ark:" + out))
            assert r.returncode == 0 and list(got) == [n for n, _, _ in items], r.stderr
            for n, x, w in items:
                exact(got[n], x, w if weighted else None, f"shapes/{tag}/{n}")
                data[f"shapes/{tag}/{n}"] = got[n]
        # d40: per speaker and global
        items = [(name_of(T, D),) + utt(T, D) for T, D in D40]
        spk = os.path.join(tmp, "spk2utt")
        open(spk, "w").write(spk2utt_text())
        by_name = {n: (x, w) for n, x, w in items}
        for weighted in (False, True):
            tag = "w" if weighted else "u"
            r, out = run(tmp, "d40s_" + tag, items, weighted, ["--spk2utt=ark:" + spk])
            got = dict(kaldi_io.read_mat64_table("ark:" + out))
            assert sorted(got) == ["spkA", "spkB"], r.stderr
            for s, ulist in SPK2UTT[:2]:
                want = sum(restate(by_name[u][0], by_name[u][1] if weighted else None) for u in ulist if u in by_name)
                assert np.array_equal(got[s], want), f"d40/{tag}/{s}: not an exact case"
                data[f"d40/{tag}/{s}"] = got[s]
            data[f"d40/{tag}/spk_counts"] = np.array(counts(r))
            data[f"d40/{tag}/spk_warnings"] = json.dumps([l.split(") ", 1)[1] for l in r.stderr.splitlines() if l.startswith("WARNING")])
            r, out = run(tmp, "d40g_" + tag, items, weighted, out=os.path.join(tmp, f"d40g_{tag}.mat"))
            g = kaldi_io.read_mat_file(out)
            want = sum(restate(x, w if weighted else None) for _, x, w in items).astype(np.float32)
            assert g.dtype == np.float32 and np.array_equal(g, want), f"d40/{tag}/global: not an exact case"
            data[f"d40/{tag}/global"] = g
            data[f"d40/{tag}/global_counts"] = np.array(counts(r))
        # bytes the reference wrote, for the writers: the per-utterance table of the two smallest utterances (binary and text), the
        # global matrix (binary and text), and the weights archive it read
        small = [(name_of(T, D),) + utt(T, D) for T, D in SHAPES[:2]]
        for mode, spec in (("bin", "ark:"), ("txt", "ark,t:")):
            r, out = run(tmp, "small_" + mode, small, False, out=spec + os.path.join(tmp, f"small_{mode}_dm.ark"))
            data["bytes/dm_" + mode] = np.frombuffer(open(out, "rb").read(), np.uint8)
        for mode, flag in (("bin", "--binary=true"), ("txt", "--binary=false")):
            r, out = run(tmp, "smallg_" + mode, small[1:], False, [flag], out=os.path.join(tmp, f"smallg_{mode}.mat"))
            data["bytes/global_" + mode] = np.frombuffer(open(out, "rb").read(), np.uint8)
        data["bytes/weights"] = np.frombuffer(b"".join(fv_entry(n, w) for n, _, w in small), np.uint8)
        # all weights missing: nothing done, exit status 1
        feats = os.path.join(tmp, "small_bin.ark")
        empty_w = os.path.join(tmp, "none_w.ark")
        open(empty_w, "wb").close()
        r = subprocess.run([tool, "--weights=ark:" + empty_w, "ark:" + feats, "ark:" + os.path.join(tmp, "none.ark")], capture_output=True, text=True)
        data["none/counts"] = np.array(counts(r))
        # the batches of 33
        for T, D in LONG:
            items = b33(T, D)
            for weighted in (False, True):
                tag = "w" if weighted else "u"
                r, out = run(tmp, f"b33_{T}x{D}_{tag}", items, weighted)
                got = list(kaldi_io.read_mat64_table("ark:" + out))
                assert [k for k, _ in got] == [n for n, _, _ in items], r.stderr
                for (k, m), (n, x, w) in zip(got, items):
                    exact(m, x, w if weighted else None, f"b33_{T}x{D}/{tag}/{n}")
                data[f"b33_{T}x{D}/{tag}/hash"] = matrices_hash([m for _, m in got])
        # wide: held to the bound, not to the bits
        x, w = wide_utt()
        for weighted in (False, True):
            tag = "w" if weighted else "u"
            r, out = run(tmp, "wide_" + tag, [("wide", x, w)], weighted)
            got = dict(kaldi_io.read_mat64_table("ark:" + out))["wide"]
            assert np.all(np.abs(got - restate(x, w if weighted else None)) <= order_bound(x, w if weighted else None)), "wide: the reference misses the bound"
            data[f"wide/{tag}"] = got
    np.savez_compressed(path, **data)


if __name__ == "__main__":
    import sys
    write_golden(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(GOLDEN), "..", "..", "oracle", "_ref", "featbin"))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
