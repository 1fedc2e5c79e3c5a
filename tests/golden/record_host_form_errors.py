"""Records host_form_errors.json: the return code and ntru_last_error() text that the built library gives to every bad-argument
case of tests/host_forms.py (needs a GPU: an engine has to exist).  The committed table was recorded from the commit before the
host forms were derived from one description each; record again only when a message is changed on purpose.

    python tests/golden/record_host_form_errors.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as ge          # noqa: E402
import host_forms as hf               # noqa: E402


def record():
    pkg = ge.load_package()
    eng, multi = pkg.Engine(0), pkg.MultiEngine([0, 0, 0])
    table = {f.name: hf.run_error_cases(eng._lib, f, eng._h) for f in hf.FORMS}
    table.update({f.name: hf.run_error_cases(multi._lib, f, multi._h) for f in hf.MULTI_FORMS})
    multi.close(), eng.close()
    return table


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "host_form_errors.json")
    with open(path, "w") as fh:
        json.dump(record(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %s" % path)
