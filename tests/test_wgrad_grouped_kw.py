"""fused_step._WGRAD_GROUPED -> the ``wgrad_grouped=`` keyword of
hip.fused_step_bf16 (no GPU needed)."""

from ray_shuffling_data_loader_amd.models import fused_step as fs


def test_default_passes_nothing(monkeypatch):
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 0)
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", None)
    assert fs._wgrad_kw() == {}


def test_override_is_passed_as_int(monkeypatch):
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 0)
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", False)
    assert fs._wgrad_kw() == {"wgrad_grouped": 0}
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", True)
    assert fs._wgrad_kw() == {"wgrad_grouped": 1}
    monkeypatch.setattr(fs, "_WGRAD_VARIANT", 2)
    monkeypatch.setattr(fs, "_WGRAD_GROUPED", None)
    assert fs._wgrad_kw() == {"wgrad_variant": 2}
