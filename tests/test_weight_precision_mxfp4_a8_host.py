"""'weightPrecision': "mxfp4-a8" of the hf model properties: parsed under both spellings, an unknown value refused with the old text and the new
value, and the value refused by name for a family other than Mistral / Llama before anything reaches a device.  No GPU."""
import json

import pytest
import torch

from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel, HuggingFaceModelProperties

BASE = {"type": "hf", "name": "some-dir", "dimensions": 128}


def test_mxfp4_a8_parses_and_an_unknown_value_names_the_five():
    for props in ({"weightPrecision": "mxfp4-a8"}, {"weight_precision": "mxfp4-a8"}):
        assert HuggingFaceModelProperties(**BASE, **props).weight_precision == "mxfp4-a8"
    with pytest.raises(ValueError, match="^'weightPrecision' must be 'bf16' or 'e4m3' or 'mxfp4' or 'mxfp4-only' or 'mxfp4-a8', got 'int4'"):
        HuggingFaceModelProperties(**BASE, weightPrecision="int4")


def test_a_bert_checkpoint_refuses_mxfp4_a8_by_name(tmp_path):
    from safetensors.torch import save_file
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="bert", vocab_size=100, max_position_embeddings=64, hidden_size=128, num_hidden_layers=2,
                                                          num_attention_heads=2, intermediate_size=256, hidden_act="gelu", layer_norm_eps=1e-12)))
    save_file({"x": torch.zeros(1)}, str(tmp_path / "model.safetensors"))
    model = HuggingFaceModel(dict(BASE, name=str(tmp_path), weightPrecision="mxfp4-a8"), device="cuda")
    with pytest.raises(InvalidModelPropertiesError, match="'weightPrecision': 'mxfp4-a8' is available for Mistral / Llama checkpoints only"):
        model._load_necessary_components()
