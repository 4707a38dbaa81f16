"""Are the gfx950 code objects of two builds the same kernels?  python probes/code_object_diff.py <libdir A> <libdir B> [--rename REGEX REPL] [--allow-added] [--classify]
(no GPU needed)

For every library (*.so) of the two directories - e.g. pontryagin-differentiable-programming_amd/lib of a checkout of the parent commit and of the working tree,
both after __graft_entry__.build() - the code object is unbundled (codegen.code_object_text) and compared:
  (a) the set of symbols in the disassembly (kernels and device functions) is the same;
  (b) per symbol the instruction text is the same.  The trailing `// address: encoding` comment of a line is dropped (a kernel may sit elsewhere in the code object
      when the host code instantiates the templates in another order), and for the same reason the literal of the s_add_u32 / s_addc_u32 pair directly behind an
      s_getpc_b64 is masked: a pc-relative offset to constant data.  Every other operand of every instruction must agree;
  (c) per kernel the metadata entry (registers, spills, scratch, LDS, kernel arguments) is the same text.
Exit status 1 on any difference.  What a host-only change of csrc/*.hip is checked with: profiles/launch_layer_code_object_diff.txt.
--rename REGEX REPL: re.sub on every symbol name of both sides before they are compared - for a change that gives a kernel template one more parameter with a default,
which changes the mangled name of the instantiations it leaves alone and must change nothing else of them.  --allow-added: symbols that only B has are counted, not
failed - what a change that ADDS instantiations is checked with (profiles/sysid_gn_code_object_diff.txt).  What follows the last kernel of a code object (the
disassembler's `...` for padding, the footer of the metadata) belongs to no kernel and is dropped: a kernel that is the last one in A need not be in B.
--ignore-trailing-nops: the run of `s_nop 0` behind the last instruction of a symbol - the assembler's padding up to the alignment of the next function of the same
section, behind an s_endpgm or an unconditional branch and never executed - is dropped on both sides: for a kernel that becomes a template instantiation, which gets a
section of its own and with it no such padding (profiles/lm_prior_code_object_diff.txt).
--classify: for every symbol whose instructions differ, one more line with generic counts - the instruction count of both sides, the number of changed lines of a
sequence match, the difference of the opcode multisets (the first word of every instruction) and whether the metadata entry is the same text: what a change that
moves kernel text into shared helpers is judged by (profiles/sysid_shared_body_code_object_diff.txt).  The exit status stays 1 on any difference."""
import collections
import difflib
import glob
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pdp_amd import codegen  # noqa: E402


RENAME = None           # (compiled regex, replacement)
IGNORE_TRAILING_NOPS = False


def renamed(name):
    return RENAME[0].sub(RENAME[1], name) if RENAME else name


def symbols(dis):
    """{symbol: [instruction text]} with the comments dropped and the pc-relative literals masked; how many literals were masked"""
    out, cur, after_getpc, masked = {}, None, 0, 0
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur, after_getpc = out.setdefault(renamed(m.group(1)), []), 0
            continue
        ins = ln.split("//")[0].strip()
        if cur is None or not ins or ins == "...":
            continue
        if after_getpc and re.match(r"s_addc?_u32 ", ins):
            ins, after_getpc, masked = re.sub(r",\s*\S+$", ", <pcrel>", ins), after_getpc - 1, masked + 1
        else:
            after_getpc = 2 if ins.startswith("s_getpc_b64") else 0
        cur.append(ins)
    if IGNORE_TRAILING_NOPS:
        for body in out.values():
            while body and body[-1] == "s_nop 0":
                body.pop()
    return out, masked


def metadata(notes):
    out = {}
    for ent in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s*(\S+)", ent).group(1)
        out[renamed(name)] = ent.split("amdhsa.target:")[0].rstrip().replace(name, renamed(name))          # (.name and .symbol carry the mangled name)
    return out


def classify(a, b):
    """generic counts of two instruction lists that differ: 'n_a -> n_b instructions, k lines changed, opcodes: same multiset | {opcode: count in b - count in a}'"""
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
    ca, cb = (collections.Counter(i.split()[0] for i in x) for x in (a, b))
    delta = {k: cb[k] - ca[k] for k in sorted(set(ca) | set(cb)) if cb[k] != ca[k]}
    ops = "same multiset" if not delta else " ".join("%s %+d" % kv for kv in delta.items())
    return "%d -> %d instructions, %d lines changed, opcodes: %s" % (len(a), len(b), changed, ops)


def main(dir_a, dir_b, allow_added=False, do_classify=False):
    names = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.so"))) for d in (dir_a, dir_b)]
    bad = int(names[0] != names[1])
    if bad:
        print("DIFFERENT sets of libraries: %s" % sorted(set(names[0]) ^ set(names[1])))
    for lib in sorted(set(names[0]) & set(names[1])):
        (na, da), (nb, db) = (codegen.code_object_text(os.path.join(d, lib)) for d in (dir_a, dir_b))
        (sa, masked), (sb, _) = symbols(da), symbols(db)
        ma, mb = metadata(na), metadata(nb)
        extra = ""
        if allow_added:
            new = [s for s in sb if s not in sa]
            sb, mb = {k: v for k, v in sb.items() if k in sa}, {k: v for k, v in mb.items() if k in ma}
            extra = "  (+%d symbols that only B has)" % len(new) if new else ""
        moved = list(sa) != list(sb)
        diffs = ["symbol set: %s" % sorted(set(sa) ^ set(sb))] if set(sa) != set(sb) else []
        diffs += ["instructions of %s" % s for s in sa if s in sb and sa[s] != sb[s]]
        diffs += ["kernel set of the metadata: %s" % sorted(set(ma) ^ set(mb))] if set(ma) != set(mb) else []
        diffs += ["metadata of %s" % s for s in ma if s in mb and ma[s] != mb[s]]
        print("%-52s %3d kernels %4d symbols %8d instructions %5d pc-relative literals masked  order %s  %s"
              % (lib, len(ma), len(sa), sum(len(v) for v in sa.values()), masked, "moved" if moved else "same ", ("DIFFERENT" if diffs else "identical") + extra))
        for d in diffs:
            print("    " + d)
        if do_classify:
            for sym in sa:
                if sym in sb and sa[sym] != sb[sym]:
                    print("    classify %s: %s, metadata %s" % (sym, classify(sa[sym], sb[sym]), "same" if ma.get(sym) == mb.get(sym) else "DIFFERENT"))
        bad += len(diffs)
    print("code objects %s" % ("DIFFER" if bad else "identical: same symbols, same instructions, same metadata in every library"))
    return 1 if bad else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--rename" in argv:
        i = argv.index("--rename")
        RENAME = (re.compile(argv[i + 1]), argv[i + 2])
        del argv[i:i + 3]
    allow = "--allow-added" in argv
    IGNORE_TRAILING_NOPS = "--ignore-trailing-nops" in argv
    do_classify = "--classify" in argv
    argv = [a for a in argv if a not in ("--allow-added", "--ignore-trailing-nops", "--classify")]
    sys.exit(main(argv[0], argv[1], allow, do_classify))
