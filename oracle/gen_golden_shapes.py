"""State-dict layout fixture: the parameter and buffer names and shapes of the REFERENCE's own modules, for the constructor arguments
tests/test_cpu_abi.py::test_mirror_state_dicts_equal_reference_modules builds the mirror modules with.  Data only (names and shapes), so
the test needs no reference checkout:

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_shapes.py <reference checkout>     # the directory that holds dmel_codec/

writes tests/golden/state_dict_shapes.json."""
from __future__ import annotations

import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "state_dict_shapes.json")

# name -> constructor arguments, shared with the test (WaveNet: input, output, residual channels, layers, dilation cycle, ...)
WAVENETS = {"wavenet_enc": [10, None, 70, 20, 4], "wavenet_cond": [64, 20, 64, 3, 4, False, 64]}
CONVNEXTS = {"convnext": [70]}
BIGVGANS = ["base_24k_100band"]


def layout(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def main(ref: str) -> None:
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(ref))      # the reference's dmel_codec must win over the alias package
    sys.dont_write_bytecode = True
    from dmel_codec.models.modules.wavenet import WaveNet
    from dmel_codec.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec.models.modules.bigvgan.env import AttrDict
    from dmel_codec.models.modules.firefly import ConvNeXtBlock
    import dmel_codec
    assert not dmel_codec.__file__.startswith(ROOT), "imported the alias package, not the reference"
    from dmel_codec_amd.configs import BIGVGAN
    out = {"meta": {"ref": "models/modules/wavenet.py, models/modules/firefly.py, models/modules/bigvgan/bigvgan.py",
                    "what": "state_dict() names -> shapes of the reference's modules"}}
    for name, a in WAVENETS.items():
        out[name] = {"args": a, "state_dict": layout(WaveNet(*a))}
    for name, a in CONVNEXTS.items():
        out[name] = {"args": a, "state_dict": layout(ConvNeXtBlock(*a))}
    for name in BIGVGANS:
        m = BigVGAN(AttrDict(dict(BIGVGAN[name])))
        before = layout(m)
        m.remove_weight_norm()
        out["bigvgan_" + name] = {"h": name, "state_dict": before, "state_dict_without_weight_norm": layout(m)}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
