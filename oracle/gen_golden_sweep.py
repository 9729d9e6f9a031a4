"""TEST INFRASTRUCTURE - generates tests/golden/sweep_characterization.json: what tracking/evaluate.py's sweep(), flag_line(), the
four table formatters and main() give under the fakes of tests/sweep_fakes.py, for the cases listed there.  No GPU is needed.

    python oracle/gen_golden_sweep.py

The fixture pins behaviour; it is generated from the code BEFORE a change to the sweep's host logic and then left alone, and
tests/test_sweep_host.py compares the code after the change against it, text for text."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'sweep_characterization.json')


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import sweep_fakes
    with tempfile.TemporaryDirectory() as directory:
        items = sweep_fakes.run_cases(directory)
    with open(OUT, 'wt') as fp:
        json.dump(items, fp, sort_keys=True, indent=0)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(items), 'items')


if __name__ == '__main__':
    main()
