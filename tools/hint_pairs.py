"""The synthetic sequence behind the hint experiments (csrc/pagk_prio.h): BASELINE configs[1]'s scene and keypoints,
seven frame pairs that differ in the camera's rotation rate and in the gyro's error -- what changes from pair to pair for a tracker
that follows the same patches.  Pair 0 is configs[1] itself.  tools/iter_trace.py <cfg> <n> <out> <pair> extracts a pair's
per-level iteration counts (oracle, CPU); tools/prio_fluid_model.py feeds pair j's totals to pair j + 1 as the hint;
tools/hint_sequence.py steps the resident tracker through the same pairs on the GPU."""
PAIRS = [
    # (omega rad/s, gyro error rad)
    ((0.5, -1.0, 2.0), (0.004, -0.003, 0.006)),
    ((0.7, -0.6, 1.6), (0.003, -0.005, 0.004)),
    ((0.2, -1.3, 2.3), (-0.002, -0.004, 0.007)),
    ((-0.4, -0.9, 1.1), (0.005, 0.002, 0.003)),
    ((0.9, 0.3, 0.8), (-0.004, 0.004, 0.005)),
    ((0.6, 0.8, -1.2), (0.002, 0.005, -0.006)),
    ((-0.3, 1.1, -1.9), (0.006, -0.002, -0.004)),
]


def workload(synth, cfg: int, n: int, pair: int):
    omega, err = PAIRS[pair]
    return synth.config(cfg, n=n, omega=omega, gyro_error=err)
