"""The evaluation driver's host side (videoloop3d_amd.evaluations; scripts/script_evaluate_ours.py): the metrics.txt layout and the
compute_img_metric drop-in's refusals -- no GPU needed."""
import numpy as np
import pytest
import torch

from videoloop3d_amd import evaluations as E

# script_evaluate_ours.py:201-204 and 249-252, spelt out
PATCH, STRIDE, PATCHT, STRIDET = [5, 11, 17], [2, 4, 6], [7, 5, 3], [1, 1, 1]
NAMES = (["name", "nnf", "nnb", "dyn", "lpips", "lpips_sw", "loop", "psnr", "ssim"]
         + [f"nnf_p{p}s{s}pt{pt}st{st}" for p, s, pt, st in zip(PATCH, STRIDE, PATCHT, STRIDET)]
         + [f"nnb_p{p}s{s}pt{pt}st{st}" for p, s, pt, st in zip(PATCH, STRIDE, PATCHT, STRIDET)]
         + [f"loop_p{p}s{s}pt{pt}st{st}" for p, s, pt, st in zip(PATCH, STRIDE, PATCHT, STRIDET)])


def _results(V, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(V):
        r = {"dyn": float(rng.uniform(0, 50)), "psnr": float(rng.uniform(15, 35)), "ssim": float(rng.uniform(0.5, 1)), "lpips": 0.0, "lpips_sw": 0.0}
        for t in ("nnf", "nnb", "loop"):
            vals = [float(x) for x in rng.uniform(1, 20, 3)]
            for c, x in zip(E.EVAL_PATCH_CONFIGS, vals):
                r[f"{t}_{E._config_tag(c)}"] = x
            r[t] = sum(vals) / len(vals)
        out.append(r)
    return out


def test_configs_are_the_scripts():
    assert E.EVAL_PATCH_CONFIGS == tuple(zip(PATCH, STRIDE, PATCHT, STRIDET)) and E.EVAL_MACRO_BLOCK == 65
    assert E.metric_names() == NAMES


@pytest.mark.parametrize("V", [1, 3])
def test_metrics_txt_layout(tmp_path, V):
    res = _results(V, seed=V)
    path = tmp_path / "eval_metrics.txt"
    E.write_metrics_txt(str(path), "fall", res)
    text = path.read_text()
    assert text.endswith("\n")
    lines = text.split("\n")[:-1]
    assert lines[0] == ", ".join(NAMES)
    assert len(lines) == V + 2
    mean = lambda x: sum(x) / len(x)
    tags = [E._config_tag(c) for c in E.EVAL_PATCH_CONFIGS]
    for i, r in enumerate(res):
        comp, coh, lq = ([r[f"{t}_{g}"] for g in tags] for t in ("nnf", "nnb", "loop"))
        want = ([f"fall_view{i}"] + [str(float(x)) for x in [mean(comp), mean(coh), r["dyn"], 0.0, 0.0, mean(lq), r["psnr"], r["ssim"]]]
                + [str(float(x)) for x in comp + coh + lq])
        assert lines[1 + i].split(", ") == want
    # the dataset row: the script's accumulation (:257-294)
    n = len(tags)
    fw, bw, lp = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
    for r in res:
        comp, coh, lq = ([r[f"{t}_{g}"] for g in tags] for t in ("nnf", "nnb", "loop"))
        fw[:n] += comp
        fw[-1] += mean(comp)
        bw[:n] += coh
        bw[-1] += mean(coh)
        lp[:n] += lq
        lp[-1] += mean(lq)
    fw, bw, lp = fw / V, bw / V, lp / V
    want = (["fall"] + [str(float(x)) for x in [fw[-1], bw[-1], mean([r["dyn"] for r in res]), 0.0, 0.0, lp[-1],
                                                mean([r["psnr"] for r in res]), mean([r["ssim"] for r in res])]]
            + [str(float(x)) for x in fw[:-1].tolist() + bw[:-1].tolist() + lp[:-1].tolist()])
    row = lines[-1].split(", ")
    assert row == want and len(row) == len(NAMES)


def test_compute_img_metric_refusals():
    a = torch.arange(2 * 8 * 9 * 3, dtype=torch.float64).reshape(2, 8, 9, 3) % 256 / 255
    m = torch.ones(1, 8, 9)
    with pytest.raises(ValueError):
        E.compute_img_metric(a, a + 0.3 / 255, "psnr", m)           # not k/255
    with pytest.raises(ValueError):
        E.compute_img_metric(a + 1.0, a, "ssim", m)                 # k/255 but k > 255
    with pytest.raises(NotImplementedError):
        E.compute_img_metric(a, a, "lpips", m)
    with pytest.raises(NotImplementedError):
        E.compute_img_metric(a, a, "psnr", m, range01=False)
    with pytest.raises(RuntimeError):
        E.compute_img_metric(a, a, "fid", m)
    with pytest.raises(NotImplementedError):
        E.evaluate_views(None, [], np.zeros((0, 4, 4)), np.zeros((0, 3, 3)), lpips=True)
