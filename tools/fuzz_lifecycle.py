"""The lifecycle fuzz of the paged MX-FP4 cache (tests/mxfp4_lifecycle.py) over many more seeds and longer
schedules than the suite replays: every schedule ``(seed, P)`` for seed in [first, last) and P in {64, 256}, every
third one on a smoothed pool, on the real ``PagedKVFP4`` with the model's check after every operation.

    python tools/fuzz_lifecycle.py 200 500 --ops 80
    python tools/fuzz_lifecycle.py 200 500 --ops 80 --steps     (decode steps among the operations)

A failed check is logged with the operations up to it and the run goes on with the next schedule; any other
error (a failed launch, the device) ends the run at once.  Prints the failures, the worst distances to the
float64 restatements per mode and the time.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mxfp4_lifecycle as LC  # noqa: E402
from test_gpu_mxfp4_lifecycle import Backend  # noqa: E402
from quantizedattention_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("--ops", type=int, default=80, help="operations per schedule")
    ap.add_argument("--steps", action="store_true", help="draw decode steps too, eager and graph-replayed")
    ap.add_argument("--seconds", type=float, default=400.0, help="start no schedule after this long")
    args = ap.parse_args()
    _lib.load()
    t0, failed, ran, worst = time.time(), 0, 0, {}
    for seed in range(args.first, args.last):
        if time.time() - t0 > args.seconds:
            break
        for P in (64, 256):
            sp = LC.spec(seed, P, args.ops, seed % 3 == 0, args.steps)
            ops = LC.schedule(seed, P, args.ops, sp.smoothed, args.steps)
            h = LC.Harness(Backend(), sp, log=lambda *_: None)
            ran += 1
            try:
                h.run(ops)
                h.operators()
            except LC.CheckFailed as e:
                failed += 1
                print(f"FAILED seed={seed} P={P} smoothed={sp.smoothed} at operation {h.n}: {e}")
                print("    " + " | ".join(LC.name_of(o) for o in ops[:h.n + 1]), flush=True)
            for mode, w in h.worst.items():
                worst[mode] = [max(a, b) for a, b in zip(worst.get(mode, (0, 0, 0)), w)]
    for mode, (o, lse, rel) in sorted(worst.items()):
        print(f"worst {mode}: O {o:.3e} lse {lse:.3e} relL2 {rel:.3e}")
    print(f"{failed} of {ran} schedules of {args.ops} operations failed, {time.time() - t0:.0f} s")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
