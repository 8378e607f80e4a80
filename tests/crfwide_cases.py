"""TEST INFRASTRUCTURE: the case list of the wide CRF kernels (csrc/crf_wide.hip, 65 <= T <= 192), shared by
tests/test_crfwide_cpu.py (which asserts that the list's tie inputs do tie and that float32 and float64 Viterbi agree on it, so the
GPU test cannot pass vacuously) and tests/test_gpu_crf_wide_kernels.py (which runs the kernels on it).

Cases are crfref case tuples (T, start, stop, B, n, emission scale, +-30 outliers); inputs, references and the check are
crfref.grid_inputs / grid_reference / check_grid, unchanged.  The widths are where a wave boundary (65, 127, 128, 129, 191, 192), the
backward kernel's template switch (128 | 129) or the limit (192) sits; 96, 137 (a 33-type BIOES dictionary) and 160 lie between.
"""
import crfref

# (T, START / STOP placement, B, n)
_WIDE = [
    (65, "last2", 3, 7), (65, "ends", 16, 48), (65, "first2", 2, 130), (65, "swapped", 5, 1), (65, "middle", 1, 1),
    (96, "middle", 16, 48), (96, "swapped", 3, 7),
    (127, "ends", 2, 130), (127, "last2", 16, 48),
    (128, "last2", 16, 48), (128, "first2", 3, 7), (128, "swapped", 2, 130), (128, "ends", 5, 1),
    (129, "ends", 16, 48), (129, "middle", 3, 7), (129, "first2", 2, 130),
    (137, "last2", 16, 48), (137, "middle", 2, 130),
    (160, "swapped", 3, 7), (160, "ends", 16, 48),
    (191, "middle", 16, 48), (191, "swapped", 2, 130),
    (192, "last2", 16, 48), (192, "first2", 2, 130), (192, "swapped", 3, 7), (192, "ends", 5, 1), (192, "middle", 1, 1),
]
WIDE = [(T,) + crfref._placements(T)[p] + (B, n, 2.0, False) for T, p, B, n in _WIDE]
WIDE += [(137, 27, 28, 3, 7, 8.0, True), (192, 17, 5, 16, 48, 8.0, True)]              # scale 8, +-30: the max-subtraction

# crfref.GRID cases that the WIDE entry points also take (1 <= T <= 192), one placement per width: both kernel families on the
# same device buffers
_NARROW = [(3, "last2", 3, 7), (29, "last2", 16, 48), (33, "first2", 2, 130), (64, "swapped", 2, 130)]
NARROW = [(T,) + crfref._placements(T)[p] + (B, n, 2.0, False) for T, p, B, n in _NARROW]
assert all(c in crfref.GRID for c in NARROW)
