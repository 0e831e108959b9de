#!/usr/bin/env python3
"""Accounts for the error texts of a unit after a refactor of the host side of the C-ABI.

    python tools/error_texts.py PARENT_FILE NEW_FILE [NEW_FILE ...]      (e.g. <(git show REV:rts_amd/csrc/rts_cube_api.hip) and the new units)

Every string literal that PARENT_FILE hands to rts_set_error must be present in the new files, unchanged (as the literal of a call or
as the sentence an entry point hands a helper) or formed from the entry point's name and the old wording ("rts_x: ..." as "%s: ...");
and no literal handed to rts_set_error in the new files may be other than a parent's wording.  Prints the counts and what is
unaccounted for or new; exit 1 if there is any."""
import re
import sys

LITERAL = r'"(?:[^"\\]|\\.)*"'


def main(argv):
    if len(argv) < 2:
        print(__doc__); return 2
    old = open(argv[0]).read(); new = "".join(open(p).read() for p in argv[1:])
    called = re.compile(r"rts_set_error\(\s*(%s)" % LITERAL)
    parent = called.findall(old); present = set(re.findall(LITERAL, new))
    with_who = lambda s: '"%s' + s[s.index(":"):] if ":" in s else s
    unchanged = [s for s in parent if s in present]
    formed = [s for s in parent if s not in present and with_who(s) in present]
    lost = [s for s in parent if s not in present and with_who(s) not in present]
    known = set(parent) | set(with_who(s) for s in parent)
    fresh = sorted(s for s in set(called.findall(new)) if s not in known)
    print("%d literals in the parent (%d distinct): %d unchanged, %d formed from who and the old wording, %d unaccounted, %d new" %
          (len(parent), len(set(parent)), len(unchanged), len(formed), len(lost), len(fresh)))
    for s in lost:
        print("  UNACCOUNTED", s)
    for s in fresh:
        print("  NEW", s)
    return 1 if lost or fresh else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
