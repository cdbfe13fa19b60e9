"""CPU: the host side of the repeated-example study (resolution_comparison_statistical): the seeded draws against
the reference's (tests/golden statistical_fixture: np.random.seed(7), its solve_multi_resolution(40, [80, 160])
three times in sequence), the summary table against numpy, and the text summary's line formats."""
import re
import sys

import numpy as np

from state import load_fixture


def _stats(a):
    return np.array([a.mean(), a.std(), np.linalg.norm(a), a.min(), a.max()])


def test_draw_fields_reproduces_reference_draws():
    from superresolution_for_pdes_amd.resolution_comparison_statistical import draw_fields
    z = load_fixture("statistical")
    np.random.seed(7)
    d = draw_fields(3, 40, [80, 160])
    assert np.array_equal(d["k1"], z["k1"]) and np.array_equal(d["k2"], z["k2"])
    assert ((d["k1"] >= 8) & (d["k1"] <= 12) & (d["k2"] >= 8) & (d["k2"] <= 12)).all()
    x = np.linspace(0, 1, 160)
    X, Y = np.meshgrid(x, x)
    for r in (40, 80, 160):
        assert d["f"][r].shape == (3, r, r) and d["theta"][r].shape == (3, r, r)
        assert d["f"][r].flags.c_contiguous and d["theta"][r].flags.c_contiguous
        step = 160 // r
        for e in range(3):
            # the same draws, so the same values: the statistics are those of identical arrays
            assert np.allclose(_stats(d["theta"][r][e]), z[f"theta{r}_stats"][e], rtol=1e-14, atol=0), (r, e)
            f = np.sin(d["k1"][e] * 2 * np.pi * X) * np.sin(d["k2"][e] * 2 * np.pi * Y)
            assert np.array_equal(d["f"][r][e], f[::step, ::step])
            assert np.array_equal(d["theta"][r][e], d["theta"][160][e][::step, ::step])


def _synthetic(n=5, resolutions=(80, 160, 320)):
    from superresolution_for_pdes_amd.resolution_comparison_statistical import METHODS
    rng = np.random.default_rng(3)
    out = []
    for e in range(n):
        m = {"example": e + 1, "k1": 9.0 + e, "k2": 10.5, "resolutions": list(resolutions)}
        for key, _ in METHODS:
            for s in ("mae", "rmse", "times"):
                m[f"{key}_{s}"] = list(rng.uniform(1e-6, 1e-3, len(resolutions)))
        m["solve_times"] = list(rng.uniform(1e-3, 1.0, len(resolutions)))
        out.append(m)
    return out


def test_summarize_equals_numpy():
    from superresolution_for_pdes_amd.resolution_comparison_statistical import METHODS, summarize
    ms = _synthetic()
    table = summarize(ms)
    assert list(table) == [80, 160, 320]
    for i, res in enumerate((80, 160, 320)):
        assert list(table[res]) == [label for _, label in METHODS]
        for key, label in METHODS:
            for name, s in (("MAE", "mae"), ("RMSE", "rmse")):
                v = np.array([m[f"{key}_{s}"][i] for m in ms])
                got = table[res][label][name]
                assert got == {"mean": float(v.mean()), "std": float(v.std(ddof=1)), "min": float(v.min()),
                               "max": float(v.max())}
    # the reference's three methods alone (its metric dicts have no cubic keys); one example: std is NaN, as pandas
    ref_only = [{k: v for k, v in ms[0].items() if not k.startswith("cubic")}]
    t1 = summarize(ref_only)
    assert list(t1[80]) == ["ML Multi-level", "Bilinear Multi-level", "Direct Bilinear"]
    assert np.isnan(t1[80]["ML Multi-level"]["MAE"]["std"]) and t1[80]["ML Multi-level"]["MAE"]["mean"] == ms[0]["ml_mae"][0]


def test_write_summary_files_and_line_formats(tmp_path):
    import csv
    import json
    from superresolution_for_pdes_amd.resolution_comparison_statistical import METHODS, summarize, write_summary
    ms = _synthetic(4, (80, 160))
    write_summary(ms, tmp_path / "out")
    text = (tmp_path / "out" / "statistical_summary.txt").read_text()
    lines = text.split("\n")
    assert lines[0] == "Statistical Summary of 4 Examples" and lines[1] == "=" * 50
    num = r"\d+\.\d{6}"
    for res in (80, 160):
        assert f"\nResults for {res}x{res} Resolution:\n" + "-" * 40 + "\n" in text
    blocks = re.findall(rf"\n(.+):\n  MAE:  mean = {num} ± {num}\n        min = {num}, max = {num}\n"
                        rf"  RMSE: mean = {num} ± {num}\n        min = {num}, max = {num}\n", text)
    assert blocks == [label for _, label in METHODS] * 2
    table = summarize(ms)
    want = table[80]["ML Multi-level"]["MAE"]
    assert f"  MAE:  mean = {want['mean']:.6f} ± {want['std']:.6f}\n        min = {want['min']:.6f}, max = {want['max']:.6f}\n" in text
    rows = list(csv.reader(open(tmp_path / "out" / "statistical_summary.csv")))
    assert rows[0] == ["", ""] + ["MAE"] * 4 + ["RMSE"] * 4
    assert rows[1] == ["", ""] + ["mean", "std", "min", "max"] * 2
    assert rows[2][:2] == ["Resolution", "Method"] and len(rows) == 3 + 2 * len(METHODS)
    first = rows[3]
    assert first[0] == "80" and first[1] == "Bilinear Multi-level"
    assert float(first[2]) == round(table[80]["Bilinear Multi-level"]["MAE"]["mean"], 6)
    assert float(first[9]) == round(table[80]["Bilinear Multi-level"]["RMSE"]["max"], 6)
    js = json.load(open(tmp_path / "out" / "statistical_summary.json"))
    assert js["n_examples"] == 4 and len(js["examples"]) == 4
    assert js["summary"]["160"]["Direct Cubic"]["RMSE"] == table[160]["Direct Cubic"]["RMSE"]


def test_module_imports_without_plot_or_table_libraries(monkeypatch):
    """With pandas, seaborn and matplotlib made unimportable the module still imports (afresh) and tabulates."""
    import importlib
    for n in ("pandas", "seaborn", "matplotlib", "matplotlib.pyplot"):
        monkeypatch.setitem(sys.modules, n, None)
    monkeypatch.delitem(sys.modules, "superresolution_for_pdes_amd.resolution_comparison_statistical", raising=False)
    S = importlib.import_module("superresolution_for_pdes_amd.resolution_comparison_statistical")
    t = S.summarize([{"resolutions": [80], "ml_mae": [1.0], "ml_rmse": [2.0]},
                     {"resolutions": [80], "ml_mae": [3.0], "ml_rmse": [2.0]}])
    assert t[80]["ML Multi-level"]["MAE"] == {"mean": 2.0, "std": float(np.std([1.0, 3.0], ddof=1)), "min": 1.0,
                                               "max": 3.0}
    src = open(S.__file__).read()
    assert not re.findall(r"^\s*(?:import|from)\s+(pandas|seaborn|matplotlib)\b", src, flags=re.M)
