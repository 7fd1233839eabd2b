"""gstex_amd.train: the means' learning-rate schedule and the preset table.  CPU only (the loop itself runs on the
GPU: tests/test_gpu_init.py)."""
import math

import pytest

from gstex_amd.model import LRS
from gstex_amd.train import PRESETS, exponential_decay


@pytest.mark.parametrize("lr_init, lr_final, max_steps",
                         [(5 * 1.6e-5, 5 * 1.6e-6, 15000), (2 * 1.6e-4, 2 * 1.6e-6, 30000), (1e-3, 5e-5, 7)])
def test_exponential_decay(lr_init, lr_final, max_steps):
    f = exponential_decay(lr_init, lr_final, max_steps)
    assert f(0) == pytest.approx(lr_init, rel=1e-15)
    assert f(max_steps) == pytest.approx(lr_final, rel=1e-15)
    assert f(2 * max_steps) == f(max_steps)
    assert f(-5) == f(0)
    assert f(max_steps / 2) == pytest.approx(math.sqrt(lr_init * lr_final), rel=1e-14)
    # the scheduler's expression itself (engine/schedulers.py:134-137, warmup_steps = 0), at an odd step
    t = 1234 / max_steps if 1234 < max_steps else 1.0
    assert f(1234) == pytest.approx(math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t), rel=1e-15)
    steps = [f(s) for s in range(0, max_steps + 1, max(max_steps // 50, 1))]
    assert all(a > b for a, b in zip(steps, steps[1:]))  # strictly decreasing up to max_steps


def test_presets_are_the_six_of_the_reference():
    assert sorted(PRESETS) == ["blender-init", "blender-lod", "blender-nvs", "colmap-init", "dtu-lod", "dtu-nvs"]
    for name, p in PRESETS.items():
        assert set(p["lrs"]) == set(LRS), name  # the seven groups
        for key in ("pixel_num", "background", "fix_init", "fix_lod_init", "max_steps", "xyz_lr_final",
                    "xyz_max_steps"):
            assert key in p, (name, key)
        assert {k: v for k, v in p["lrs"].items() if k != "xyz"} == {k: v for k, v in LRS.items() if k != "xyz"}
        assert 0 < p["xyz_lr_final"] < p["lrs"]["xyz"]
        assert p["background"] == ("white" if "blender" in name else "black")
        assert p["fix_init"] == ("blender" not in name)
    assert PRESETS["blender-nvs"]["lrs"] == LRS  # model.LRS is that preset (gstex_configs.py:207-244)
    assert PRESETS["blender-nvs"]["xyz_lr_final"] == 5 * 1.6e-6 and PRESETS["blender-nvs"]["xyz_max_steps"] == 15000
    assert PRESETS["dtu-lod"]["fix_lod_init"] and not PRESETS["blender-lod"]["fix_lod_init"]
    assert PRESETS["dtu-lod"]["lrs"]["xyz"] == 2 * 1.6e-4 and PRESETS["dtu-lod"]["xyz_max_steps"] == 30000
    assert PRESETS["colmap-init"]["pixel_num"] == 1e7 and PRESETS["dtu-nvs"]["pixel_num"] == 1e6
    assert [PRESETS[k]["max_steps"] for k in ("blender-init", "blender-nvs", "blender-lod")] == [1, 15000, 7000]


def test_trainer_takes_a_preset_s_learning_rates():
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene

    sc = make_scene(50, 500, seed=1)
    tr = GStexTrainer(sc, "cpu", fused_adam=False, lrs=PRESETS["dtu-lod"]["lrs"])
    assert {g["name"]: g["lr"] for g in tr.optimizer.param_groups} == PRESETS["dtu-lod"]["lrs"]
    assert {g["name"]: g["lr"] for g in GStexTrainer(sc, "cpu", fused_adam=False).optimizer.param_groups} == LRS
    with pytest.raises(ValueError, match="lrs"):
        GStexTrainer(sc, "cpu", fused_adam=False, lrs={"xyz": 1e-4})


class _RecordingTrainer:
    """The calls fit makes, recorded: a stand-in with the trainer's step interface (no rendering)."""

    def __init__(self, start_step=0):
        import torch

        self.device = torch.device("cpu")
        self.lrs = dict(LRS)
        self.step = start_step
        self.optimizer = type("O", (), {})()
        self.optimizer.param_groups = [{"name": n, "lr": lr} for n, lr in LRS.items()]
        self.calls = []

    def _lr(self, name):
        return next(g["lr"] for g in self.optimizer.param_groups if g["name"] == name)

    def zero_grad(self):
        self.calls.append(("zero_grad", self.step))

    def forward_backward(self, view, image, mask=None):
        import torch

        self.calls.append(("forward_backward", self.step, view.tag, int(image[0]), mask))
        return type("Out", (), {"loss": torch.tensor(float(self.step) + 0.25)})()

    def optimizer_step(self):
        self.calls.append(("optimizer_step", self.step, self._lr("xyz"), self._lr("texture_dc")))
        self.step += 1

    def recharge(self):
        self.calls.append(("recharge", self.step))


class _View:
    def __init__(self, tag):
        self.tag = tag

    def to(self, device):
        return self


def test_fit_makes_the_calls_of_the_hand_written_loop():
    """Deterministic counterpart of tests/test_gpu_init.py's numerical comparison: per step s, in this order, the
    xyz lr of the schedule, zero_grad, forward_backward on the drawn pair, optimizer_step, then recharge when
    s % build_chart_every == 0 -- from the trainer's step counter, so a resumed run continues the schedule."""
    import torch

    from gstex_amd.train import fit

    pairs = [(_View(k), torch.tensor([k])) for k in range(3)]
    tr = _RecordingTrainer(start_step=8)
    seen = []
    res = fit(tr, pairs, 7, xyz_lr_final=1e-6, max_steps=20, build_chart_every=5, seed=3,
              on_step=lambda s, out: seen.append((s, float(out.loss))))
    f = exponential_decay(LRS["xyz"], 1e-6, 20)
    want = []
    for i, k in enumerate(res["views"]):
        s = 8 + i
        want += [("zero_grad", s), ("forward_backward", s, k, k, None), ("optimizer_step", s, f(s), LRS["texture_dc"])]
        if s % 5 == 0:
            want.append(("recharge", s + 1))  # (after the optimizer step: the counter has advanced)
    assert tr.calls == want
    assert res["recharts"] == [10] and tr.step == 15
    assert seen == [(8 + i, 8 + i + 0.25) for i in range(7)]
    assert res["loss"].tolist() == [8 + i + 0.25 for i in range(7)]
    gen = torch.Generator().manual_seed(3)
    perms = [torch.randperm(3, generator=gen).tolist() for _ in range(3)]
    assert res["views"] == (perms[0] + perms[1] + perms[2])[:7]
    # no schedule: the lr is left alone; build_chart_every=0: never a rechart; a mask is passed through
    tr = _RecordingTrainer()
    mask = torch.ones(1, dtype=torch.bool)
    res = fit(tr, [(_View(0), torch.tensor([0]), mask)], 3, build_chart_every=0)
    assert [c for c in tr.calls if c[0] == "optimizer_step"] == [("optimizer_step", s, LRS["xyz"], LRS["texture_dc"])
                                                                 for s in range(3)]
    assert res["recharts"] == [] and all(c[4] is mask for c in tr.calls if c[0] == "forward_backward")
    with pytest.raises(ValueError, match="pairs"):
        fit(_RecordingTrainer(), [], 1)
