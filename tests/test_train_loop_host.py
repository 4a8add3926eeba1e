"""CPU: the host side of must3r_amd/train.py -- ``select_batch`` and ``get_args_parser`` against what the reference's own functions returned
(tests/golden/select_batch_cases.json, recorded by scripts/make_train_fixture.py; live against the reference where its tree exists), the logger, the loss value
taken from the details, the refusals and ``save_final_model``."""
import functools
import importlib.util
import json
import math
import os
import types

import pytest
import torch

from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import losses as L, train as T


@functools.lru_cache(maxsize=None)
def _maker():
    spec = importlib.util.spec_from_file_location("make_train_fixture", os.path.join(ROOT, "scripts", "make_train_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(os.path.join(GOLDEN, "select_batch_cases.json")) as f:
        return json.load(f)


def _ours():
    parser = T.get_args_parser()
    return [dict(case=c, result=_maker().run_case(T.select_batch, parser, c)) for c in _maker().grid()]


def _compare(ours, theirs, same_torch):
    assert len(ours) == len(theirs) == 4 * 2 * 2 * 2 * 3 * 4
    for a, b in zip(ours, theirs):
        assert a["case"] == b["case"]
        ra, rb = dict(a["result"]), dict(b["result"])
        if not same_torch:          # torch.randperm's stream belongs to the torch version: hold what does not depend on it
            for r in (ra, rb):
                r.pop("next_randperm")
                r["to_render"] = None if r["to_render"] is None else len(r["to_render"])
        assert ra == rb, (a["case"], ra, rb)


def test_the_grid_takes_every_branch():
    res = [c["result"] for c in _fixture()["cases"]]
    cases = [c["case"] for c in _fixture()["cases"]]
    assert any(r["to_skip"] > 0 for r in res) and any(r["to_skip"] == 0 and c["memory_num_views"] < c["nimgs"] for r, c in zip(res, cases))
    assert any(r["to_render"] is None for r in res) and any(r["to_render"] == [] for r in res) and any(r["to_render"] for r in res)
    assert any(len(r["kept"]) < c["nimgs"] for r, c in zip(res, cases)) and any(len(r["to_skip_batches"]) > 1 for r in res)
    assert {c["memory_num_views"] for c in cases} == {2, 3, 6, 10} and {c["progress"] for c in cases} == {0.0, 0.5, 1.0} and {c["seed"] for c in cases} == {0, 1, 2, 3}
    assert os.path.getsize(os.path.join(GOLDEN, "select_batch_cases.json")) < 256 * 1024


def test_select_batch_returns_what_the_reference_recorded():
    fx = _fixture()
    same = fx["torch_version"].split("+")[0].split(".")[:2] == torch.__version__.split("+")[0].split(".")[:2]
    _compare(_ours(), fx["cases"], same)
    if HAS_REFERENCE:               # the same grid, live against the reference's function
        from oracle.ref_shims import REFERENCE_ROOT
        live = _maker().build(REFERENCE_ROOT)
        _compare(_ours(), live["cases"], True)
        assert _maker().parser_table(T.get_args_parser()) == live["parser"]
        assert json.loads(json.dumps(live["parser"])) == fx["parser"]


def test_parser_has_the_references_options_and_defaults():
    table = json.loads(json.dumps(_maker().parser_table(T.get_args_parser())))
    ref = _fixture()["parser"]
    assert table["prog"] == ref["prog"] and table["add_help"] == ref["add_help"] and table["exclusive"] == ref["exclusive"]
    assert [o["dest"] for o in table["options"]] == [o["dest"] for o in ref["options"]]
    for a, b in zip(table["options"], ref["options"]):
        assert a == b, (a, b)
    args = T.get_args_parser().parse_args(["--dataset", "x"])
    assert args.amp is False and args.accum_iter == 2 and args.memory_num_views == 10 and args.criterion == T.DEFAULT_CRITERION
    with pytest.raises(SystemExit):
        T.get_args_parser().parse_args([])                                                   # --dataset is required
    with pytest.raises(SystemExit):
        T.get_args_parser().parse_args(["--dataset", "x", "--render_once", "--disable_render"])
    ok = T.get_args_parser().parse_args(["--dataset", "x", "--use_memory_efficient_attention", "--disable_cudnn_benchmark", "--disable_tf32", "--amp", "bf16"])
    assert ok.amp == "bf16" and ok.disable_tf32


def test_logger_averages():
    log = T.MetricLogger()
    seen = []
    for i, x in enumerate(log.log_every([10, 20, 30], 2, "head")):
        seen.append(x)
        log.update(loss=float(x), lr=0.5 / (i + 1))
        log.update(epoch=i / 3, skipped=None)
        log.update(t=torch.tensor(2.0 * x))
    assert seen == [10, 20, 30] and set(log.meters) == {"loss", "lr", "epoch", "t"}
    assert log.meters["loss"].global_avg == (10.0 + 20.0 + 30.0) / 3 and log.meters["loss"].count == 3 and log.meters["loss"].value == 30.0
    assert log.meters["lr"].global_avg == (0.5 + 0.25 + 0.5 / 3) / 3 and log.meters["t"].global_avg == 40.0
    assert "loss: 20.0000" in str(log)
    with pytest.raises(AssertionError):
        log.update(bad="text")


def test_loss_value_comes_from_the_details_in_fp32():
    crit = L.ConfLoss(L.Regr3D(L.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)
    g, l = float(torch.tensor(0.1, dtype=torch.float32)), float(torch.tensor(1.7, dtype=torch.float32))
    loss = torch.tensor(g, dtype=torch.float32) + torch.tensor(l, dtype=torch.float32)

    class Unread(torch.Tensor):
        def __float__(self):
            raise AssertionError("the loss was read")
    unread = loss.as_subclass(Unread)
    assert T.loss_value_from_details(crit, unread, dict(conf_loss_g=g, conf_loss_l=l)) == float(loss) != g + l
    assert T.loss_value_from_details(crit, unread, dict(conf_loss_g=g)) == g
    assert math.isinf(T.loss_value_from_details(crit, unread, dict(conf_loss_g=float("inf"), conf_loss_l=l)))
    assert math.isnan(T.loss_value_from_details(crit, unread, dict(conf_loss_g=float("inf"), conf_loss_l=float("-inf"))))
    assert T.loss_value_from_details(crit, unread, dict(conf_loss_g=3e38, conf_loss_l=3e38)) == float("inf")      # fp32 overflow, as the device's sum
    # anything else is read
    assert T.loss_value_from_details(object(), loss, {}) == float(loss)
    crit._alpha = 0.5
    assert T.loss_value_from_details(crit, loss, dict(conf_loss_g=g, conf_loss_l=l)) == float(loss)


def _args(**kw):
    a = T.get_args_parser().parse_args(["--dataset", "x"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refusals():
    none = types.SimpleNamespace(train=lambda *_: None)
    with pytest.raises(NotImplementedError, match="fp16"):
        T.train_one_epoch(none, none, None, [], None, "cpu", 0, None, _args(amp="fp16"))
    with pytest.raises(NotImplementedError, match="DDP"):
        T.train_one_epoch(none, none, None, [], None, "cpu", 0, None, _args(world_size=2))
    with pytest.raises(NotImplementedError, match="DDP"):
        T.check_single_process(_args(dist_on_itp=True))
    T.check_single_process(_args())


def test_save_final_model(tmp_path):
    enc, dec = torch.nn.Linear(2, 2), {"w": torch.ones(3)}
    path = T.save_final_model(_args(output_dir=str(tmp_path)), 20, enc, dec)
    assert path == tmp_path / "checkpoint-final.pth"
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"args", "encoder", "decoder", "epoch"} and ck["epoch"] == 20 and ck["args"].output_dir == str(tmp_path)
    assert torch.equal(ck["encoder"]["weight"], enc.weight) and torch.equal(ck["decoder"]["w"], dec["w"])
