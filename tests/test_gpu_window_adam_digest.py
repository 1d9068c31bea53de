"""optim.WindowAdam computes the bits it computed before its C ABI was folded into one `vl3d_adam_window` argument: the sha256 of the parameter,
both moments and the per-tile step table after every step of tests/window_adam_scenario.py, on five storages, against
tests/golden/window_adam_digest.json -- recorded by tests/golden/make_window_adam_digest.py on the MI355X at the commit before that change."""
import json
import os

import pytest
import torch

import window_adam_scenario as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_adam_digest.json")


@pytest.mark.parametrize("storage", S.STORAGES)
def test_window_adam_digest(storage):
    want = json.load(open(GOLDEN))[storage]
    got = S.run(storage, torch.device("cuda:0"))
    assert len(got["steps"]) == len(want["steps"]) == (13 if storage.startswith("packed") else 14)
    for t, (g, w) in enumerate(zip(got["steps"], want["steps"]), 1):
        assert g == w, f"{storage}: step {t} differs in {[k for k in w if g[k] != w[k]]}"
    assert got["final"] == want["final"], f"{storage}: after flush() / state_dict()"
