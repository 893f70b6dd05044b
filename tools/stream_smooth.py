"""Per-push time of a BlockStream over Smooth(x, 5 ms), 8 channels, blocks of 48000 frames, against one sink of such a block
(profiles/r19/stream_smooth.txt).  `python tools/stream_smooth.py [out.json]` on the GPU; prints one JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sigops_amd as so

FS, NCH, BLOCK, PUSHES = 48 * so.kHz, 8, 48_000, 220
torch.manual_seed(1)
blocks = [torch.randn((BLOCK, NCH), dtype=torch.float64, device="cuda") for _ in range(4)]
pipe = lambda s: so.Smooth(s, 5 * so.ms)  # noqa: E731


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


# the floor: one sink of one block's Smooth, device array to device result (a plan, its launches, a check), warmed up
planar = blocks[0].t().contiguous().t()
floor = [timed(lambda: so.sink(pipe(so.Signal(planar, FS)), "torch"))[0] for _ in range(60)][10:]
runs = []
for rep in range(2):
    bs = so.BlockStream(pipe, FS, nch=NCH)
    ms = []
    for k in range(PUSHES):
        t, out = timed(lambda: bs.push(blocks[k % 4]))
        ms.append(t)
    assert bs.emitted == PUSHES * BLOCK - 1 and bs.start > 0
    runs.append(ms)
ms = runs[1]  # (the first stream also pays the first launches of every kernel)
res = {"block": BLOCK, "nch": NCH, "pushes": PUSHES,
       "sink_one_block_ms_median": statistics.median(floor), "sink_one_block_ms_min": min(floor),
       "first_stream_push_1_ms": runs[0][0], "push_1_ms": ms[0], "push_2_ms": ms[1], "push_200_ms": ms[199],
       "pushes_2_to_20_ms_median": statistics.median(ms[1:20]), "pushes_181_to_220_ms_median": statistics.median(ms[180:]),
       "pushes_181_to_220_ms_max": max(ms[180:])}
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res))
