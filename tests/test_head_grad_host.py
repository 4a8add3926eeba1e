"""CPU: the host side of the prediction head's training path -- the ABI 19 surface, the yardstick's indexing, the split rule and the refusals
of must3r_amd.train_head (no compute calls: no GPU here)."""
import ctypes as C

import pytest
import torch

import head_ref as HR
from must3r_amd import _lib, train_head as TH


def test_abi_19_symbols_and_signatures():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION >= 19
    for name in ("must3r_hip_head_grad_splits", "must3r_hip_head_forward_scratch_bytes", "must3r_hip_head_forward", "must3r_hip_op_head_linear",
                 "must3r_hip_head_grad_scratch_bytes", "must3r_hip_head_grad", "must3r_hip_op_linear_dgrad_f32",
                 "must3r_hip_op_linear_wgrad_scratch_bytes", "must3r_hip_op_linear_wgrad_f32", "must3r_hip_op_layernorm_grad_scratch_bytes",
                 "must3r_hip_op_layernorm_grad"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    # the descriptor: five inputs, four sizes, eps and a reserved word, five outputs
    assert [f[0] for f in _lib.HeadGradArgs._fields_] == ["x", "gamma", "beta", "W", "G", "n_views", "H", "Wimg", "D", "eps", "reserved",
                                                          "dx", "dgamma", "dbeta", "dW", "db"]
    assert C.sizeof(_lib.HeadGradArgs) == 5 * 8 + 6 * 4 + 5 * 8


def test_scratch_queries_answer_without_a_device():
    lib = _lib.load()
    big = lib.must3r_hip_head_grad_scratch_bytes(28 * 20, 384, 512, 768)
    assert 0 < big < 28 * 20 * 384 * 512 * 7 * 4          # below the size of the upstream gradient itself
    assert lib.must3r_hip_head_grad_scratch_bytes(1, 32, 48, 768) > 0
    for bad in ((1, 40, 48, 768), (1, 32, 50, 768), (1, 32, 48, 96), (0, 32, 48, 768)):
        assert lib.must3r_hip_head_grad_scratch_bytes(*bad) == 0, bad
        assert lib.must3r_hip_head_forward_scratch_bytes(*bad) == 0, bad
    assert b"multiples of 16" in (lib.must3r_hip_head_grad_scratch_bytes(1, 40, 48, 768), lib.must3r_hip_last_error())[1]
    a = _lib.HeadGradArgs()
    assert lib.must3r_hip_head_grad(C.byref(a), None, 0, None) != 0        # refused before anything is launched
    assert lib.must3r_hip_head_grad(None, None, 0, None) != 0 and b"null" in lib.must3r_hip_last_error()


def test_pixel_shuffle_indexing_is_the_headers_formula():
    n, H, W = 2, 32, 48
    R = n * (H // 16) * (W // 16)
    z = torch.arange(R * HR.OUT, dtype=torch.int64).view(R, HR.OUT)
    fast = torch.nn.functional.pixel_shuffle(z.view(n, H // 16, W // 16, HR.OUT).permute(0, 3, 1, 2), 16).permute(0, 2, 3, 1)
    loop = HR.pixel_shuffle_loop(z, n, H, W)
    assert torch.equal(fast, loop)
    assert torch.equal(HR.unshuffle(loop), z)             # the backward's gather inverts it
    x = torch.randn(R, 64)
    out = HR.head(x, torch.ones(64), torch.zeros(64), torch.randn(HR.OUT, 64), torch.zeros(HR.OUT), n, H, W)
    assert out.shape == (n, H, W, 7)


def test_split_count_is_pure_and_monotone():
    lib = _lib.load()
    prev = 0
    for R in list(range(1, 4200)) + [15360, 430080, 2 ** 30]:
        s = TH.wgrad_splits(R)
        assert s == lib.must3r_hip_head_grad_splits(R) == TH.wgrad_splits(R), R
        assert 1 <= s <= TH.WGRAD_MAX_SPLITS and s >= prev, R
        prev = s
    assert TH.wgrad_splits(6) == 1 and TH.wgrad_splits(429) == 4 and TH.wgrad_splits(640) == 5 and TH.wgrad_splits(430080) == 16
    assert lib.must3r_hip_head_grad_splits(0) == 0 == TH.wgrad_splits(0)


def _params(D=64):
    return torch.ones(D), torch.zeros(D), torch.zeros(HR.OUT, D), torch.zeros(HR.OUT)


def test_refusals():
    tok = torch.zeros(2, 6, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        TH.prediction_head(tok, (32, 48), *_params())
    with pytest.raises(ValueError, match="do not match"):
        TH.prediction_head(torch.zeros(2, 5, 64), (32, 48), *_params())
    with pytest.raises(ValueError, match="multiple of 16"):
        TH.prediction_head(tok, (40, 48), *_params())
    with pytest.raises(ValueError, match="parameters"):
        TH.prediction_head(tok, (32, 48), *_params(128))
    head = TH.PredictionHead(64)
    with pytest.raises(ValueError, match="share"):
        head(tok, torch.tensor([[32, 48], [48, 32]]))
    with pytest.raises(RuntimeError, match="GPU"):
        head(tok, torch.tensor([[32, 48], [32, 48]]))


def test_state_dict_keys_are_the_references():
    head = TH.PredictionHead(128)
    sd = head.state_dict()
    assert list(sd) == ["norm_dec.weight", "norm_dec.bias", "head_dec.proj.weight", "head_dec.proj.bias"]
    assert sd["head_dec.proj.weight"].shape == (7 * 16 * 16, 128) and all(v.dtype == torch.float32 for v in sd.values())
    assert all(p.requires_grad for p in head.parameters())

    class _Dec:                                            # what from_decoder reads of a decoder
        norm_dec = torch.nn.LayerNorm(128, eps=1e-6)
        head_dec = type("H", (), {"proj": torch.nn.Linear(128, 1792)})()
    copy = TH.PredictionHead.from_decoder(_Dec)
    assert torch.equal(copy.head_dec.proj.weight, _Dec.head_dec.proj.weight) and copy.head_dec.proj.weight is not _Dec.head_dec.proj.weight
    copy.load_state_dict(sd, strict=True)
