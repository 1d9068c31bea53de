"""Records tests/golden/window_adam_digest.json: the sha256 digests of (p, m, v, last_step) after every step of the run in
tests/window_adam_scenario.py, on its five storages, as the package of a GIVEN tree computes them on the MI355X.  The committed file was
recorded at the commit before the crop-aware optimiser's entry points took one `vl3d_adam_window` argument: check that commit out into a
directory of its own, copy this file and tests/window_adam_scenario.py into it, build it there
(python -c "import __graft_entry__ as g; g.build()"), and run, in THAT checkout on the GPU machine,
    python tests/golden/make_window_adam_digest.py [OUT.json]
tests/test_gpu_window_adam_digest.py compares the current tree with the file."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import window_adam_scenario as S  # noqa: E402


def main(out):
    dev = torch.device("cuda:0")
    res = {storage: S.run(storage, dev) for storage in S.STORAGES}
    again = {storage: S.run(storage, dev) for storage in S.STORAGES}
    assert res == again, "the run is not deterministic"
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "window_adam_digest.json"))
