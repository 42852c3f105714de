"""The Philox4x32-10 reference of tests/small_kernel_refs.py against the published known-answer vectors, and its array form
against its integer form: what tests/test_small_kernels_gpu.py holds `ops.randn` to must itself be right."""
import numpy as np
import pytest

import small_kernel_refs as R

# counter, key, expected words (the known-answer vectors of the Random123 distribution for philox4x32, 10 rounds)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_known_answer_vectors(counter, key, want):
    assert R.philox4x32_10(counter, key) == want


def test_array_form_reproduces_the_first_known_answer():
    assert tuple(int(w) for w in R.philox_words(0, 0, 1)[0]) == KNOWN_ANSWERS[0][2]


@pytest.mark.parametrize("seed,offset", [(0, 0), (0, 1), (2 ** 32 + 5, 0), (2 ** 63 + 7, 2 ** 32 - 2), (123, 250000),
                                         (2 ** 64 - 1, 2 ** 64 - 3)])
def test_array_form_equals_integer_form(seed, offset):
    """Counter words {ctr_lo, ctr_hi, 0, 0}, key {seed_lo, seed_hi}; the counter crosses 2^32 (and wraps at 2^64) inside."""
    words = R.philox_words(seed, offset, 7)
    for q in range(7):
        ctr = (offset + q) & R.MASK64
        want = R.philox4x32_10((ctr & R.MASK32, ctr >> 32, 0, 0), (seed & R.MASK32, (seed >> 32) & R.MASK32))
        assert tuple(int(w) for w in words[q]) == want


def test_box_muller_mapping_of_chosen_words():
    """u1 = ((w >> 8) + 1) / 2^24 never reaches 0, u2 = (w >> 8) / 2^24 never reaches 1; the low 8 bits do not count."""
    words = np.array([[0xffffffff, 0, 0x000000ff, 0x40000000]], dtype=np.uint64)
    z = R.normals_from_words(words)
    assert z[0] == 0.0 and z[1] == 0.0                                  # u1 = 1: radius 0
    r = np.sqrt(-2.0 * np.log(2.0 ** -24))                              # u1 = 2^-24: the largest radius, about 5.77
    theta = float(np.float32(2.0 * np.pi) * np.float32(0.25))
    assert z[2] == r * np.cos(theta) and z[3] == r * np.sin(theta)
    assert 5.7 < r < 5.8
