"""Records tests/golden/factor_bits.json for tests/test_gpu_factor_bits.py: the digests of everything the factoring calls return, on the
cases of tests/factor_bits_cases.py.

Run on an MI355X with a build of the commit BEFORE csrc/eqf_factor.hpp (the parent of the commit that added it) loaded through
EQF_VIO_AMD_LIB:

    EQF_VIO_AMD_LIB=/path/to/parent/libeqf_vio_amd.so python tests/golden/make_golden_factor_bits.py [OUT.json]

Run it twice: every call here is bit-for-bit reproducible, so two recordings that differ in a digest mean a bug in a case (an input that
is not seeded, an output read before it is there), not noise.  The fixture names the library (the source hash eqf_build_info() carries)
and the compiler that built it.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import factor_bits_cases as fb  # noqa: E402
from eqf_vio_amd import binding  # noqa: E402


def main(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    ver = [ln for ln in subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.split("\n") if "version" in ln]
    doc = {"build_info": binding.lib().eqf_build_info().decode().split("=", 1)[1], "compiler": "; ".join(ver), "cases": {}}
    for name in sorted(fb.CASES):
        doc["cases"][name] = fb.CASES[name](binding)
        print(name, len(doc["cases"][name]), "fields", flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "factor_bits.json"))
