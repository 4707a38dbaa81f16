"""For every kernel whose instructions differ between two builds: instruction count, opcode multiset and metadata entry, A against B.
python probes/code_object_counts.py <libdir A> <libdir B>   (no GPU needed; the companion of probes/code_object_diff.py, which says WHICH symbols differ)

A kernel that a refactor only re-ordered has the same count, the same multiset and the same metadata.  Output appended to profiles/chain_rule_code_object_diff.txt."""
import collections
import glob
import os
import subprocess
import sys

import code_object_diff as cod
from pdp_amd import codegen


def demangled(sym):
    out = subprocess.run(["c++filt", sym], stdout=subprocess.PIPE, text=True).stdout.strip()
    return out.split("(")[0].replace("void pdp::", "")


def main(dir_a, dir_b):
    for lib in sorted(os.path.basename(p) for p in glob.glob(os.path.join(dir_b, "*.so"))):
        if not os.path.exists(os.path.join(dir_a, lib)):
            continue
        (na, da), (nb, db) = (codegen.code_object_text(os.path.join(d, lib)) for d in (dir_a, dir_b))
        (sa, _), (sb, _) = cod.symbols(da), cod.symbols(db)
        ma, mb = cod.metadata(na), cod.metadata(nb)
        for s in sa:
            if s in sb and sa[s] != sb[s]:
                oa, ob = (collections.Counter(i.split()[0] for i in x) for x in (sa[s], sb[s]))
                print("%-44s %-58s instructions %5d -> %5d  opcode multiset %-9s metadata %s" % (
                    lib[len("libpdp_model_"):-3], demangled(s), len(sa[s]), len(sb[s]), "same" if oa == ob else "different", "same" if ma.get(s) == mb.get(s) else "different"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
