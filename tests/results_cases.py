"""The rows the result ring is tested on (tests/test_sequence_results_cpu.py, tests/test_sequence_results_gpu.py): rows of
tests/sequence_cases.py by name, and one row of its own in the same format.

three-chunks-refill: 320 x 240, half patch 5, three levels, cap 2200, target 2100, 3000 candidates per frame, four frames, frame
2 constant gray.  Every track dies at the gray frame and the hand-over refills from the candidate list alone, so that frame
issues ids to new rows in all three chunks of 1024 rows while next_id is already above zero."""
from __future__ import annotations

import sequence_cases as sc

TABLE = {
    "three-chunks-refill": sc._row(320, 240, 5, 3, 2200, 2100, n_cand=3000, nf=4, gray=2),
}
LOCKSTEP = ("base", "deep-small", "cap-is-target", "smallest", "odd-gray3", "lk", "lk-gyro-harris", "pm-fast", "sensor",
            "two-rounds-pm", "three-chunks-refill")
PIPELINED = ("base", "odd-gray3", "pm-fast", "sensor", "three-chunks-refill")
LAYOUT_CAPS = (1, 4, 12, 33, 40, 70, 2200)
CHUNK = 1024   # rows a workgroup of the pack owns (csrc/pagk_results_kernel.h)


def scene(name: str) -> dict:
    """sequence_cases.scene for a row of either table (the other module's table is left as it was)."""
    if name in sc.TABLE:
        return sc.scene(name)
    sc.TABLE[name] = TABLE[name]
    try:
        return sc.scene(name)
    finally:
        del sc.TABLE[name]
