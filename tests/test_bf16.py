"""BF16 GGUF files without a GPU: the synthetic writer's tensors read back bit for bit, and the
loader's expert-type check names a BF16 expert tensor."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import random_blocks
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, tensor_plan, build_vocab, write_synthetic_gguf


@pytest.mark.parametrize("spec", ["tiny-llama-bf16", "tiny-qwen3-bf16"])
def test_synthetic_bf16_reads_back_bit_equal(tmp_path, spec):
    r = GGUFReader(write_synthetic_gguf(spec, str(tmp_path / "m.gguf"), seed=4))
    rng = np.random.default_rng(4)   # the writer's stream: tensors in plan order
    for name, t, shape in tensor_plan(SPECS[spec], build_vocab(SPECS[spec])[1]):
        n = int(np.prod(shape))
        if t != GGMLType.BF16:
            rng.standard_normal(n)   # (every F32 tensor of these specs is one normal draw per element)
            continue
        assert int(r.tensors[name].ggml_type) == GGMLType.BF16, name
        want = random_blocks(t, n, rng, std=1.0 if name == "token_embd.weight" else SPECS[spec].weight_std)
        assert np.array_equal(np.asarray(r.raw(name)).view(np.uint8).reshape(-1), want), name


def test_expert_check_names_bf16_tensor():
    from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
    with pytest.raises(RuntimeError, match=r"blk\.3\.ffn_down_exps\.weight.*BF16"):
        load_cpu().check_expert_type("blk.3.ffn_down_exps.weight", int(GGMLType.BF16))
    load_cpu().check_expert_type("blk.3.ffn_down_exps.weight", int(GGMLType.F16))   # a supported type passes
