"""Seeded random cases of kmx_spectra_* against tests/spectra_ref.py: the mode, N in 1 ... 2000, rows in 0 ... 5000, key words, the body's
shape (zero, same, skewed, uniform), the list (left out, reversed, a scattered subset, one column), both caps anywhere in their ranges
and on either side of what LDS holds, 1 ... 80 pairs with repeats and x = y, either flag alone or both, host or device-resident rows at
any byte offset, one call or two calls over a cut into the caller's tables, and the launch knobs.  Both tables are compared bit for
bit.  Needs the GPU (no fallback).
Usage: stress_spectra.py [--cases 80] [--seed 1] [--seconds 240] [--out profiles/spectra_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import spectra_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=80)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_spectra.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed = time.time(), [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode = int(rng.integers(0, 2))
        N = int(rng.choice([rng.integers(1, 132), rng.integers(1, 2001), rng.integers(2000, 6000) if mode == sr.MODE_PA else rng.integers(1, 300)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5001)]))
        rows = int(min(rows, 4_000_000 // N))
        kw = int(rng.integers(1, 5))
        shape = str(rng.choice(sr.SHAPES))
        kind = str(rng.choice(sr.KINDS))
        cols = sr.make_cols(kind, N, int(rng.integers(1 << 30)))
        M = N if cols is None else len(cols)
        cap = int(rng.choice([1, 2, rng.integers(1, 256), 254, 255, 256, rng.integers(256, 2000), 65535]))
        if M * (cap + 2) > 4_000_000:
            cap = 255
        jc = int(rng.choice([1, 2, rng.integers(1, 110), 108, 109, 110, rng.integers(110, 256), 255]))
        P = int(rng.choice([1, 2, 3, 4, 15, 16, 17, rng.integers(1, 81)]))
        if P * (jc + 1) ** 2 > 2_000_000:
            P = max(1, 2_000_000 // (jc + 1) ** 2)
        pairs = rng.integers(0, N, (P, 2)).astype(np.uint32)
        if P >= 3:
            pairs[1, 1] = pairs[1, 0]; pairs[P - 1] = pairs[0]
        want = int(rng.integers(1, 4))      # 1 HIST, 2 JOINT, 3 both
        body = sr.spectra_body(int(rng.integers(1 << 30)), rows, N, kw, mode, shape, (cap, jc))
        eh, ej = sr.spectra_expected_np(body, N, kw, mode, cols, cap, pairs, jc)
        resident, shift, two = bool(rng.integers(0, 2)), int(rng.integers(0, 8)), bool(rng.integers(0, 2)) and rows > 1
        knobs = [{}, dict(KMX_SPECTRA_CUS="1"), dict(KMX_SPECTRA_GRID="1"), dict(KMX_SPECTRA_GRID="7")][int(rng.integers(0, 4))]
        rb = sr.row_bytes(kw, N, mode)
        cuts = [0, int(rng.integers(1, rows)), rows] if two else [0, rows]
        d_h = torch.zeros((M, cap + 2), dtype=torch.int64, device=dev)
        d_j = torch.zeros((P, jc + 1, jc + 1), dtype=torch.int64, device=dev)
        buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
        buf[shift:shift + len(body)] = torch.from_numpy(np.array(body)).to(dev)
        torch.cuda.synchronize()
        os.environ.update(knobs)
        for r0, r1 in zip(cuts, cuts[1:]):
            args = dict(cols=cols, cap=cap, hist=bool(want & 1), hist_dev=d_h.data_ptr() if want & 1 else None, pairs=pairs if want & 2 else None, joint_cap=jc,
                        joint_dev=d_j.data_ptr() if want & 2 else None)
            if resident:
                ctx.spectra_dev(buf.data_ptr() + shift + r0 * rb, r1 - r0, N, kw, mode, **args)
            else:
                ctx.spectra(body[r0 * rb:r1 * rb], r1 - r0, N, kw, mode, **args)
        for k in knobs:
            del os.environ[k]
        torch.cuda.synchronize()
        got_h, got_j = d_h.cpu().numpy().view(np.uint64), d_j.cpu().numpy().view(np.uint64)
        ok = (got_h.tobytes() == eh.tobytes() if want & 1 else not got_h.any()) and (got_j.tobytes() == ej.tobytes() if want & 2 else not got_j.any())
        pl = sr.joint_plan(pairs, jc, rb)
        rec = dict(case=case, mode=["count", "pa"][mode], n_cols=N, n_use=M, cols=kind, rows=rows, key_words=kw, shape=shape, cap=cap, joint_cap=jc, pairs=P,
                   flags=want, hist_in_lds=bool(mode == sr.MODE_COUNT and cap <= sr.HIST_LDS_CAP), joint_in_lds=pl["lds"], road="stream" if pl["stream"] else "gather",
                   resident=resident, shift=shift if resident else None, calls=len(cuts) - 1, knobs=knobs, ok=bool(ok))
        done.append(rec)
        if not ok:
            failed.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    summary = dict(device=torch.cuda.get_device_name(0), seed=a.seed, cases=len(done), failed=len(failed), seconds=round(time.time() - t0, 1), runs=done)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps(dict(cases=len(done), failed=len(failed), equal=len(done) - len(failed))))
    sys.exit(1 if failed else 0)


main()
