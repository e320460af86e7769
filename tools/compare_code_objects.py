"""Compare the gfx950 kernels of two builds of libtqdne_hip.so: same instruction stream and same register / LDS / scratch metadata?

    python tools/compare_code_objects.py OLD.so NEW.so

Every kernel of OLD must be in NEW with identical machine code (the encoded instruction words, which are position independent) and
identical .vgpr_count / .sgpr_count / .agpr_count / .group_segment_fixed_size / .private_segment_fixed_size / spill counts.  Names are
compared demangled; a template argument list of NEW may carry extra trailing arguments (a new defaulted template parameter).  Kernels
only in NEW are listed.  Needs no GPU; exit status 1 on any difference.

    --rename OLD_REGEX=NEW_TEMPLATE   (repeatable) a kernel of OLD whose demangled name matches OLD_REGEX is paired with the kernel of NEW
                                      named re.sub(OLD_REGEX, NEW_TEMPLATE, name): for kernels that were renamed or whose parameter list changed

A pair whose instruction words differ gets a second look at the disassembly: "scalar argument loads only" if it is equal line for line
once the immediate offset of the s_load_* instructions is masked (a kernel argument moved), else "same mnemonics apart from s_load / s_waitcnt"
if the sequence of mnemonics is equal once those two kinds of line are dropped (scalar loads regrouped, registers renumbered)."""

import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count", ".max_flat_workgroup_size", ".kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout


def demangle(names):
    tool = shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")
    r = subprocess.run([tool], input="\n".join(names).encode(), check=True, stdout=subprocess.PIPE)
    return r.stdout.decode().splitlines()


def code_objects(so, tmp):
    """the gfx950 ELF images of every offload bundle in the library's .hip_fatbin section"""
    fat = os.path.join(tmp, os.path.basename(so) + ".fatbin")
    run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat)
    blob = open(fat, "rb").read()
    out = []
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    for n, st in enumerate(starts):
        b = blob[st:starts[n + 1] if n + 1 < len(starts) else len(blob)]
        nent = int.from_bytes(b[24:32], "little")
        pos = 32
        for _ in range(nent):
            off, size, tlen = (int.from_bytes(b[pos + 8 * i:pos + 8 * i + 8], "little") for i in range(3))
            triple = b[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, "%s.%d.co" % (os.path.basename(so), len(out)))
                open(path, "wb").write(b[off:off + size])
                out.append(path)
    return out


def kernels(so, tmp):
    """{demangled kernel name: (sha1 of the instruction words, metadata dict, instruction text lines)}"""
    res = {}
    for co in code_objects(so, tmp):
        notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).decode()
        meta = {}
        for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            blk = ".agpr_count:" + blk
            name = re.search(r"\.name:\s+(\S+)", blk).group(1).strip("'\"")
            meta[name] = {k: re.search(re.escape(k) + r":\s+(\S+)", blk).group(1) for k in META if re.search(re.escape(k) + r":\s+(\S+)", blk)}
        dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", co).decode()
        cur, h = None, None
        streams, text = {}, {}
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1)
                streams[cur] = hashlib.sha1()
                text[cur] = []
                continue
            m = re.search(r"//\s*[0-9A-Fa-f]+:\s*((?:[0-9A-Fa-f]{8}\s*)+)(?:<.*>)?\s*$", line)
            if cur and m:
                streams[cur].update(m.group(1).encode())
                text[cur].append(" ".join(line.split("//")[0].split()))
        names = list(meta)
        dem = demangle(names)
        for mangled, d in zip(names, dem):
            res[d] = (streams[mangled].hexdigest() if mangled in streams else None, meta[mangled], text.get(mangled, []))
    return res


def strip_added_args(new_name, old_names):
    """NEW name -> the OLD name it extends by trailing template arguments, or None"""
    m = re.match(r"^(.*<.*?)((?:, [^,<>]+)+)>(\(.*)$", new_name)
    while m:
        head, extra, tail = m.groups()
        parts = extra.split(", ")[1:]
        for k in range(len(parts)):
            cand = head + "".join(", " + x for x in parts[:k]) + ">" + tail
            if cand in old_names:
                return cand
        return None
    return None


def code_verdict(a, b):
    """what is left of a difference in the instruction words, from the two disassemblies"""
    def masked(t):
        return [re.sub(r"(0x[0-9a-f]+|\d+)$", "#", l) if l.startswith("s_load_") else l for l in t]

    def mnemonics(t):
        return [l.split()[0] for l in t if not l.startswith(("s_load_", "s_waitcnt"))]
    if masked(a) == masked(b):
        return "scalar argument loads only"
    if mnemonics(a) == mnemonics(b):
        return "same mnemonics apart from s_load / s_waitcnt (%d / %d instructions)" % (len(a), len(b))
    ca, cb = collections.Counter(mnemonics(a)), collections.Counter(mnemonics(b))
    return "CODE differs (%d / %d instructions; counts of other mnemonics that changed: %s)" % (
        len(a), len(b), {m: cb[m] - ca[m] for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]} or "none, order only")


def main(old_so, new_so, renames=()):
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(old_so, tmp), kernels(new_so, tmp)
    alias = {}
    for o in old:
        for rx, tpl in renames:
            n = re.sub(rx, tpl, o)
            if n != o and o not in new and n in new:
                alias.setdefault(o, []).append(n)
    for n in new:
        if n not in old:
            o = strip_added_args(n, old)
            if o is not None:
                alias.setdefault(o, []).append(n)
    bad = 0
    counterpart = {}
    for name, (h, meta, txt) in sorted(old.items()):
        # (several instantiations of NEW may extend one OLD name -- the default of the added parameter and other values of it: the one
        # that reproduces OLD is its counterpart)
        cands = [name] if name in new else alias.get(name, [])
        if not cands:
            print("MISSING in new:", name)
            bad += 1
            continue
        nn = next((c for c in cands if new[c][:2] == (h, meta)), cands[0])
        counterpart[name] = nn
        h2, meta2, txt2 = new[nn]
        if h != h2 or h is None:
            print("%s: %s -> %s" % (code_verdict(txt, txt2), name, nn))
            bad += 1
        if meta != meta2:
            print("METADATA differs:", name, {k: (meta.get(k), meta2.get(k)) for k in META if meta.get(k) != meta2.get(k)})
            bad += 1
    matched = set(counterpart.values())
    extra = sorted(n for n in new if n not in matched)
    print("%d kernels in old, %d in new, %d renamed, %d only in new, %d differences"
          % (len(old), len(new), sum(1 for k, v in counterpart.items() if k != v), len(extra), bad))
    for n in extra:
        m = new[n][1]
        print("  new: %s  [vgpr %s, sgpr %s, static lds %s, scratch %s]" % (re.sub(r"\(.*$", "", n.replace("void (anonymous namespace)::", "")),
              m.get(".vgpr_count"), m.get(".sgpr_count"), m.get(".group_segment_fixed_size"), m.get(".private_segment_fixed_size")))
    return 1 if bad else 0


if __name__ == "__main__":
    argv, renames = sys.argv[1:], []
    while "--rename" in argv:
        i = argv.index("--rename")
        renames.append(tuple(argv[i + 1].split("=", 1)))
        del argv[i:i + 2]
    sys.exit(main(argv[0], argv[1], renames))
