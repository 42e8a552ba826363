from relora_amd.ops.functional import (  # noqa: F401
    build_rope_cache,
    doc_mask,
    doc_starts_from_eos,
    flash_attention,
    gelu,
    fused_cross_entropy,
    layernorm,
    lora_group_ok,
    lora_group_rope_ok,
    lora_linear,
    lora_linear_group,
    add_rmsnorm,
    rmsnorm,
    rmsnorm_torch,
    rope,
    rope_torch,
    rotate_half,
    swiglu,
    swiglu_torch,
)
from relora_amd.ops import hip  # noqa: F401
from relora_amd.ops.optim import stochastic_round_bf16  # noqa: F401
