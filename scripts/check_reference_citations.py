"""include/gpx.h, DESIGN.md, INTEGRATION.md and the host modules cite the pybo call site each entry point replaces as
`pybo/<file>.py:<line>[-<line>]`.  Check that every cited file exists in a checkout of the reference pybo and that every
cited line is inside it.

Run:  python scripts/check_reference_citations.py <directory holding the reference's pybo/ package>
Exit code 0 when every citation resolves, 1 otherwise (one line per bad citation on stderr)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def citations():
    """{(file relative to pybo/, highest cited line)} over the header, the two documents and pybo_amd/."""
    cited = set()
    files = [os.path.join(ROOT, 'include', 'gpx.h'), os.path.join(ROOT, 'DESIGN.md'), os.path.join(ROOT, 'INTEGRATION.md')]
    for dp, _, fs in os.walk(os.path.join(ROOT, 'pybo_amd')):
        files += [os.path.join(dp, f) for f in fs if f.endswith(('.py', '.hip', '.h'))]
    for path in files:
        txt = open(path, encoding='utf-8', errors='replace').read()
        for m in re.finditer(r'pybo/([a-z_/]+\.py):(\d+)(?:-(\d+))?((?:,\d+(?:-\d+)?)*)', txt):
            nums = [int(m.group(2))] + ([int(m.group(3))] if m.group(3) else [])
            nums += [int(v) for v in re.findall(r'\d+', m.group(4) or '')]
            cited.add((m.group(1), max(nums)))
    return cited


def main(ref):
    cited = citations()
    bad = []
    if len(cited) < 20:
        bad.append('only %d citations found' % len(cited))
    for rel, last in sorted(cited):
        path = os.path.join(ref, 'pybo', rel)
        if not os.path.exists(path):
            bad.append('%s does not exist' % rel)
            continue
        n = len(open(path, encoding='utf-8', errors='replace').read().splitlines())
        if last > n:
            bad.append('%s has %d lines, cited line %d' % (rel, n, last))
    for b in bad:
        sys.stderr.write(b + '\n')
    print('%d citations checked, %d bad' % (len(cited), len(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    raise SystemExit(main(sys.argv[1]))
