"""'weightPrecision': "mxfp4" of the hf model properties: parsed, refused by name for a family other than Mistral / Llama before anything reaches a
device, and the e8m0 block-scale rule of tests/w4_ref.py at its edges.  No GPU."""
import json
from fractions import Fraction

import pytest
import torch

from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel, HuggingFaceModelProperties
from tests import w4_ref as R

BASE = {"type": "hf", "name": "some-dir", "dimensions": 128}


def test_mxfp4_parses_and_an_unknown_value_names_the_three():
    for props in ({"weightPrecision": "mxfp4"}, {"weight_precision": "mxfp4"}):
        assert HuggingFaceModelProperties(**BASE, **props).weight_precision == "mxfp4"
    with pytest.raises(ValueError, match="'weightPrecision' must be 'bf16' or 'e4m3' or 'mxfp4'"):
        HuggingFaceModelProperties(**BASE, weightPrecision="int4")


def test_a_bert_checkpoint_refuses_mxfp4_by_name(tmp_path):
    from safetensors.torch import save_file
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="bert", vocab_size=100, max_position_embeddings=64, hidden_size=128, num_hidden_layers=2,
                                                          num_attention_heads=2, intermediate_size=256, hidden_act="gelu", layer_norm_eps=1e-12)))
    save_file({"x": torch.zeros(1)}, str(tmp_path / "model.safetensors"))
    model = HuggingFaceModel(dict(BASE, name=str(tmp_path), weightPrecision="mxfp4"), device="cuda")
    with pytest.raises(InvalidModelPropertiesError, match="'weightPrecision': 'mxfp4' is available for Mistral / Llama checkpoints only \\(model_type 'bert'\\)"):
        model._load_necessary_components()


@pytest.mark.parametrize("absmax", (6.0, 6.03125, 5.96875, 3.0, 1.0, 6.0 * 2.0 ** -20, 6.03125 * 2.0 ** 20, 2.0 ** -60))
def test_scale_is_the_smallest_power_of_two_that_keeps_the_block_inside_6(absmax):
    k = R.scale_exponent(absmax)
    assert Fraction(absmax) <= 6 * Fraction(2) ** k and Fraction(absmax) > 6 * Fraction(2) ** (k - 1)


def test_zero_blocks_and_the_clamp():
    assert R.scale_exponent(0.0) == 0 and R.scale_exponent(2.0 ** -130) == -100 and R.scale_exponent(3.0e38) == 100
