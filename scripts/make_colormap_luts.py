"""Writes nerfstudio-thermal_amd/colormap_luts.json from the matplotlib installed on the build machine (data only): `names` and `luts`, float32 [6, 256, 3] in that order, as
JSON text -- every value the shortest decimal that reads back to the same float32 --: the five
listed colour maps the reference's apply_float_colormap indexes (nerfstudio/utils/colormaps.py:114: matplotlib.colormaps[name].colors, 256 rows each;
float32 is what torch.tensor(list of Python floats) makes of them there) and, last, "gray" sampled at its 256 entries (k / 255; the renderer repeats
the value for "gray" as the reference does and never reads this table: it is there for a viewer's legend).  The machines that render need no
matplotlib.

    python scripts/make_colormap_luts.py"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "nerfstudio-thermal_amd", "colormap_luts.json")
NAMES = ("turbo", "viridis", "magma", "inferno", "cividis", "gray")  # ("default" is turbo)


def main():
    import matplotlib

    def table(name):
        cmap = matplotlib.colormaps[name]
        return np.asarray(cmap.colors if hasattr(cmap, "colors") else cmap(np.arange(256))[:, :3], dtype=np.float64).astype(np.float32)

    luts = np.stack([table(name) for name in NAMES])
    assert luts.shape == (len(NAMES), 256, 3)
    rows = ",\n".join(json.dumps([[float(str(v)) for v in row] for row in table]) for table in luts)  # (str of a float32: its shortest form)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write('{"names": %s,\n "matplotlib_version": %s,\n "luts": [\n%s\n]}\n' % (json.dumps(list(NAMES)), json.dumps(matplotlib.__version__), rows))
    with open(OUT, encoding="utf-8") as f:
        assert np.array_equal(np.array(json.load(f)["luts"], dtype=np.float64).astype(np.float32), luts)  # reads back to the same bits
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, matplotlib {matplotlib.__version__}")


if __name__ == "__main__":
    main()
