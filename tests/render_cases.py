"""Note lists shared by the render tests (tests/test_render_arithmetic.py on the host, tests/test_gpu_render.py on the
device).  A note is (start, end, pitch, velocity[, is_drum])."""

RATE = 16000

# six simultaneous notes, low to high, staggered by a few ms so that attacks, decays and releases overlap: the polyphony
# the tolerance is derived for (synthetic.random_music's max_polyphony)
SIX = [(0.010, 0.260, 40, 127), (0.012, 0.300, 52, 100), (0.015, 0.240, 59, 90), (0.020, 0.280, 64, 127),
       (0.022, 0.310, 71, 80), (0.030, 0.250, 88, 110)]

# one 0.2 s note of pitch 96 that starts at 590 s of a 600 s sequence: its sixth partial has turned 7.4 million times by
# then, so time or phase in float32 is nowhere near
LATE = [(590.0, 590.2, 96, 100)]
LATE_SAMPLES = 600 * RATE
LATE_WINDOW = (590 * RATE - 8, int(590.24 * RATE) + 8)
