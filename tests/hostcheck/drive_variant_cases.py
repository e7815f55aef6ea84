"""TEST INFRASTRUCTURE.  Runs every case of tests/variant_cases.py against the stand-in HIP runtime of tests/hostcheck (kernels never run:
which variant a launcher selects is host state) and prints, per case, what the variant census (hip.variant_census) says it selected; then the
library's whole enumeration.  Run by tests/test_variant_reach_host.py in a child process; one JSON line each."""
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from solver2d_amd import hip  # noqa: E402
from tests import variant_cases  # noqa: E402


def main():
    only = set(sys.argv[1:])
    for case in variant_cases.CASES:
        if only and case.name not in only:
            continue
        try:
            got, error = sorted(variant_cases.run_case(hip, case)), None
        except Exception:  # (reported per case: the test names it)
            got, error = [], traceback.format_exc()[-1500:]
        print("CASE " + json.dumps({"name": case.name, "selected": got, "error": error}), flush=True)
    census = hip.variant_census()
    print("ENUMERATION " + json.dumps({"families": hip.variant_families(), "entries": sorted((f, k) for f, keys in census.items() for k in keys)}), flush=True)
    print("VARIANT CASES DRIVER OK", flush=True)


if __name__ == "__main__":
    main()
