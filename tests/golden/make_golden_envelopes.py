"""Extract the stored arrays of the sampled and Fourier envelope shapes from the reference's test fixture.

Run once where the reference's tests are at hand (the pickle never travels to the GPU box):

    python tests/golden/make_golden_envelopes.py

The pickle is data only; it is decoded with the unpickler stub of make_golden.py (any `tensorflow.*` global maps to
`numpy.asarray`), which runs no reference code.

Output (committed):
  envelopes.npz  <- test/envelopes.pickle: the four arrays `pwc_shape`, `pwc_symmetric`, `fourier_sin`, `fourier_cos`
                    (test_envelopes.py:33-50,84-102: the shape functions on ts = linspace(0, 10e-9, 100)), nothing else.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

NAMES = ("pwc_shape", "pwc_symmetric", "fourier_sin", "fourier_cos")


def main():
    d = make_golden.load("envelopes.pickle")
    np.savez_compressed(os.path.join(make_golden.OUT, "envelopes.npz"), **{n: np.asarray(d[n]) for n in NAMES})


if __name__ == "__main__":
    main()
