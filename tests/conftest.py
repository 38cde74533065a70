import multiprocessing
import os
import sys

import pytest

# Make the in-tree package importable when tests run from the repo root.
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires an AMD GPU (MI355X); skipped on CPU"
    )


def pytest_collection_modifyitems(config, items):
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip_gpu = pytest.mark.skip(reason="no GPU available")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip_gpu)


@pytest.fixture(scope="session", autouse=True)
def _short_queue_rendezvous_dir():
    """Named-queue tests bind Unix sockets under RSDL_QUEUE_DIR (default:
    the temp dir) and an AF_UNIX path is capped at ~107 bytes, so under a
    long TMPDIR the bind fails before any queue code runs. When the temp
    dir is long and the caller chose no rendezvous dir, use a fresh short
    one for the session (spawned trainer processes inherit it)."""
    import shutil
    import tempfile

    if (
        "RSDL_QUEUE_DIR" in os.environ
        or len(tempfile.gettempdir()) <= 24
        or not os.access("/tmp", os.W_OK)
    ):
        yield
        return
    d = tempfile.mkdtemp(prefix="rq", dir="/tmp")
    os.environ["RSDL_QUEUE_DIR"] = d
    try:
        yield
    finally:
        os.environ.pop("RSDL_QUEUE_DIR", None)
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def mp_spawn_context():
    return multiprocessing.get_context("spawn")
