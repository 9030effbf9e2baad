"""Writes tests/golden/denoise_book_64x36.npz: the 64x36 book cover (seed 2, d = 50)
from the CPU oracle, as tests/denoise_frames.py renders it: `noisy` (r = 16, pass
0), `target` (r = 1024, pass 1: independent samples) and the guides `albedo`,
`normal` and `depth` of the noisy frame's samples. tests/test_denoise_ref_cpu.py
measures the restatement's MSE on it and re-renders `noisy` to see that the file
still is what the oracle gives (the target takes the oracle ~10 s, hence a file).

    python tests/golden/make_denoise_book.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    import denoise_frames
    from oracle import oracle as O

    noisy, target, albedo, normal, depth = denoise_frames.book_cover(O, 64, 36, 16, 1024,
                                                                     workers=min(16, os.cpu_count() or 1))
    np.savez_compressed(os.path.join(HERE, "denoise_book_64x36.npz"), noisy=noisy, target=target, albedo=albedo,
                        normal=normal, depth=depth)
