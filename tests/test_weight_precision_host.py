"""'weightPrecision' of the hf model properties (parsing, default, alias) and the power-of-two scale rule of tests/w8_ref.py at its edges.  No GPU."""
import math
from fractions import Fraction

import pytest

from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModelProperties
from tests import w8_ref as R

BASE = {"type": "hf", "name": "some-dir", "dimensions": 128}


def test_weight_precision_parses_defaults_and_refuses():
    for props, want in (({}, "bf16"), ({"weightPrecision": "e4m3"}, "e4m3"), ({"weight_precision": "e4m3"}, "e4m3"), ({"weightPrecision": "bf16"}, "bf16")):
        p = HuggingFaceModelProperties(**BASE, **props)
        assert p.weight_precision == want and p.engine_precision == "bf16"
    for bad in ("int4", "fp8", "E4M3", None):
        with pytest.raises(ValueError, match="'weightPrecision' must be 'bf16' or 'e4m3'"):
            HuggingFaceModelProperties(**BASE, weightPrecision=bad)


@pytest.mark.parametrize("absmax", (448.0, 450.0, 447.0, 224.0, 1.0, 448.0 * 2.0 ** -20, 448.0 * 2.0 ** 20, 449.0 * 2.0 ** -20, 2.0 ** -60, 3.0e38))
def test_scale_is_the_smallest_power_of_two_that_keeps_the_row_inside_448(absmax):
    s = R.pow2_scale(absmax)
    k = round(math.log2(s))
    assert s == 2.0 ** k
    assert Fraction(absmax) <= 448 * Fraction(2) ** k and Fraction(absmax) > 448 * Fraction(2) ** (k - 1)


def test_zero_rows_and_the_floor():
    assert R.pow2_scale(0.0) == 1.0 and R.pow2_scale(2.0 ** -130) == 2.0 ** -100
