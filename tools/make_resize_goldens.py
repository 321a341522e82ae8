"""Write tests/golden/resize_crop_pil_sha256.json: the SHA-256 of Pillow's resize + centre crop of each case in
tests/resize_ref.GOLDEN_CASES (sources from resize_ref.source_image), so that the GPU tests pin Pillow's bytes where Pillow
is not installed.  Needs Pillow; run from the repository root: python tools/make_resize_goldens.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import resize_ref as R  # noqa: E402


def main():
    import PIL
    cases = []
    for seed, h, w, c, rs, crop, f in R.GOLDEN_CASES:
        crop_bytes = R.pil_resize_crop(R.source_image(seed, h, w, c), rs, crop, R.FILTERS[f])
        cases.append({"seed": seed, "height": h, "width": w, "channels": c, "resize_short": rs, "crop": crop, "filter": f,
                      "sha256": R.sha256(crop_bytes)})
    out = ROOT / "tests" / "golden" / "resize_crop_pil_sha256.json"
    out.write_text(json.dumps({"pillow": PIL.__version__, "layout": "hwc", "cases": cases}, indent=1) + "\n")
    print(f"wrote {out} ({len(cases)} cases, Pillow {PIL.__version__})")


if __name__ == "__main__":
    main()
