"""CPU test of the RSDL_CHAIN_ROWS latch of models/fused_step.py: at the
default (0) no ``rows`` keyword reaches the chain bindings, so stand-ins
without the argument (tests/_fake_hip.py) keep working; a set value is
passed through."""

from ray_shuffling_data_loader_amd.models import fused_step as fs


def test_rows_kw_follows_latch(monkeypatch):
    monkeypatch.setattr(fs, "_CHAIN_ROWS", 0)
    assert fs._rows_kw() == {}
    for rows in (32, 64):
        monkeypatch.setattr(fs, "_CHAIN_ROWS", rows)
        assert fs._rows_kw() == {"rows": rows}
