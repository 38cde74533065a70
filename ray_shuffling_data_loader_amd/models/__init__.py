"""Models and train-step schedules for the MI355X loader's benchmarks."""

from ray_shuffling_data_loader_amd.models.fused_optim import (  # noqa: F401
    FusedOptimizer,
)
