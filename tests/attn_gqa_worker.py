"""Child-process worker for tests/test_gpu_attention_gqa.py: the
RELORA_AMD_ATTN_* / RELORA_AMD_DQ_* flags are read once per process, so each
environment-selected instantiation needs a fresh process.

`python tests/attn_gqa_worker.py [--hd128]` runs one grouped-query case
(B=2, nh=4, nkv=2, S=320, hd=64; with --hd128 also hd=128) through
`attn_fwd`/`attn_bwd` under whatever flags its environment carries and
prints one JSON line of error/bound ratios; the parent asserts the bounds.
"""

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_variant_worker as aw  # noqa: E402
import gqa_common as gc  # noqa: E402


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd.ops import hip

    ext = hip.ext()
    assert ext is not None, "HIP extension not built"
    assert torch.cuda.is_available(), "gqa worker needs a GPU"
    out = {}
    for hd in ((64, 128) if "--hd128" in argv else (64,)):
        q, k, v, dout = gc.make_inputs(2, 4, 2, 320, hd)
        ref = gc.ref_gqa(q, k, v, dout)
        got = aw.run_kernels(ext, *(t.cuda() for t in (q, k, v, dout)))
        torch.cuda.synchronize()
        assert got["dk"].shape == k.shape and got["dv"].shape == v.shape
        out[f"nkv2_S320_hd{hd}"] = aw.all_ratios(got, ref)
    print("ATTN_GQA_RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
