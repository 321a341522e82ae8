"""Write tests/golden/box_resize_pil_sha256.json: the SHA-256 of Pillow's Image.resize((out, out), filter, box=box) of each
case in tests/box_ref.GOLDEN_CASES (sources from resize_ref.source_image), so that the GPU tests pin Pillow's bytes where
Pillow is not installed.  Needs Pillow; run from the repository root: python tools/make_box_goldens.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import box_ref as B  # noqa: E402


def main():
    import PIL
    cases = []
    for seed, h, w, c, box, out, f in B.GOLDEN_CASES:
        crop_bytes = B.pil_resize_box(B.source_image(seed, h, w, c), box, out, B.FILTERS[f])
        cases.append({"seed": seed, "height": h, "width": w, "channels": c, "box": [float(v) for v in box], "out": out,
                      "filter": f, "sha256": B.sha256(crop_bytes)})
    path = ROOT / "tests" / "golden" / "box_resize_pil_sha256.json"
    path.write_text(json.dumps({"pillow": PIL.__version__, "layout": "hwc", "cases": cases}, indent=1) + "\n")
    print(f"wrote {path} ({len(cases)} cases, Pillow {PIL.__version__})")


if __name__ == "__main__":
    main()
