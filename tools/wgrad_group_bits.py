"""Digest what the grouped weight-gradient launch (grappa_gemm_f32_grouped) writes on the cases of tests/wgrad_group_cases.py: SHA-256 of
every member's dW and db, per case (operand formats x finishing route).  An output's bits depend on the case's inputs alone, so two builds
of the library that compute the same thing give the same digests.

    python tools/wgrad_group_bits.py --write-golden        # ONCE, on the library a change starts from: tests/golden/wgrad_group_bits.json
    python tools/wgrad_group_bits.py --out profiles/wgrad_group_bits.txt      # the loaded library beside the golden column; exit 1 if they differ

(GRAPPA_HIP_LIB selects the library: grappa_amd/settings.py.)  tests/test_gpu_wgrad_group_bits.py gates on the golden file, which is never
regenerated from the code under test.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wgrad_group_cases as wc      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_group_bits.json")


def current(lib):
    out = {}
    for group in wc.GROUPS:
        g = wc.Group(lib, group)
        inputs = wc.input_digest(group)
        for route in wc.ROUTES:
            rc, outs, ws_ok, _ = g.run(route)
            if rc != 0 or not ws_ok:
                sys.exit(f"wgrad_group_bits: {wc.case_id(group, route)}: status {rc}, workspace guard {'intact' if ws_ok else 'WRITTEN'}")
            out[wc.case_id(group, route)] = {"inputs": inputs, "outputs": g.digests(outs)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write-golden", action="store_true")
    ap.add_argument("--golden", default=GOLDEN)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wgrad_group_bits: needs a GPU")
    from grappa_amd import _lib
    now = current(_lib.load())
    if args.write_golden:
        os.makedirs(os.path.dirname(os.path.abspath(args.golden)), exist_ok=True)
        with open(args.golden, "w") as f:
            json.dump(now, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {args.golden}: {len(now)} cases from {_lib.LIB_PATH}")
        return
    with open(args.golden) as f:
        gold = json.load(f)
    lines = [f"# case, output: digest of the library the change started from (tests/golden/wgrad_group_bits.json) | digest of this library | same?"]
    bad = 0
    for cid in sorted(now):
        lines.append(cid)
        want, got = gold.get(cid, {"inputs": "-", "outputs": {}}), now[cid]
        rows = [("inputs", want["inputs"], got["inputs"])] + [(k, want["outputs"].get(k, "-"), v) for k, v in sorted(got["outputs"].items())]
        for name, w, g in rows:
            bad += w != g
            lines.append(f"  {name:22s} {w[:32]} | {g[:32]} | {'same' if w == g else 'DIFFERENT'}")
    lines.append(f"# {len(now)} cases, {bad} digests differ")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
