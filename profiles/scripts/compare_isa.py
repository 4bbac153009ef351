"""Two-listing comparison of a library build against another build of it, kernel by kernel.

    python profiles/scripts/compare_isa.py A_DIR A_LOG B_DIR B_LOG [name-prefix ...] > table.txt
    python profiles/scripts/compare_isa.py --kd A/libmcba.so B/libmcba.so       # the *.kd symbols of both libraries

A_DIR / B_DIR: the device listing of every translation unit of a tree, written as UNIT-hip-amdgcn-amd-amdhsa-gfx950.s by
    hipcc <the flags of multical_amd/build.py> -Rpass-analysis=kernel-resource-usage --cuda-device-only -S csrc/UNIT.hip -o DIR/UNIT-...s
(NOT -save-temps: compiling from the preprocessed source selects other instructions in k_linearize than the library build does).
A_LOG / B_LOG: what those compilations printed (the resource remarks).
Prints (1) whether both builds hold the same kernels, (2) per kernel whose listing or resource figures differ the figures A | B,
the instruction counts and the differing instruction lines by kind:
  commuted  same opcode and destination, the same source operands in another order
  inverted  a scalar compare or the branch on it, replaced by its opposite (s_cmp_eq <-> s_cmp_lg, scc0 <-> scc1, ...)
  other     anything else
and (3) per kernel family (all that differ + those whose name starts with one of the prefixes) how many instantiations are identical.
"""
import difflib
import glob
import os
import re
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]
SHORT = ["VGPR", "AGPR", "SGPR", "Sspill", "Vspill", "scratch", "LDS", "occ"]
INVERSE = [("s_cmp_eq", "s_cmp_lg"), ("s_cmp_lt", "s_cmp_ge"), ("s_cmp_gt", "s_cmp_le"), ("s_cbranch_scc0", "s_cbranch_scc1"),
           ("s_cbranch_vccz", "s_cbranch_vccnz"), ("s_cbranch_execz", "s_cbranch_execnz")]


def symbol(name):
  """(a kernel of internal linkage carries an L before its own name, _ZN4mcba7handeyeL10k_hand_eye..: static or not, it is the same kernel)"""
  return re.sub(r"L(\d+k_)", r"\1", name)


def listings(build_dir):
  """kernel symbol -> {unit: list of instruction lines} (comments and directives dropped, labels kept out).  The symbol alone
  is the key: a kernel that moved to another translation unit is the same kernel."""
  out = {}
  for path in sorted(glob.glob(os.path.join(build_dir, "*-gfx950.s"))):
    name, body = None, []
    for line in open(path):
      m = re.match(r"^(\w+):", line)
      if m and not line.startswith(".L"):
        name, body = symbol(m.group(1)), []
        continue
      if name is None:
        continue
      if line.startswith(".Lfunc_end"):
        out.setdefault(name, {})[os.path.basename(path).split("-hip-")[0]] = body
        name = None
        continue
      text = line.split(";")[0].strip()
      if text and not text.startswith(".") and not text.endswith(":"):
        # (block labels carry the function's number in the listing: .LBB12_3 -> .LBB_3)
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", text)))
  return out


def kernels_of(build_dir):
  """the kernel descriptor symbols of the build's listings -> the units that emit them"""
  names = {}
  for path in glob.glob(os.path.join(build_dir, "*-gfx950.s")):
    unit = os.path.basename(path).split("-hip-")[0]
    for line in open(path):
      m = re.match(r"^\s*\.amdhsa_kernel\s+(\w+)", line)
      if m:
        names.setdefault(symbol(m.group(1)), []).append(unit)
  return names


def resources(log):
  """symbol -> the figures of its remarks (one dict per translation unit that emits it)"""
  res, cur = {}, None
  for line in open(log):
    m = re.search(r"Function Name: (\w+)", line)
    if m:
      cur = res.setdefault(symbol(m.group(1)), [])
      cur.append({})
      continue
    m = re.search(r"\s{3,}([A-Za-z][^:]*): (\S+) \[-Rpass", line)
    if m and cur is not None:
      cur[-1][m.group(1).strip()] = m.group(2)
  return res


def demangle(names):
  """_ZN4mcba11k_linearizeILi5ELi0E..EEv.. -> k_linearize<5,0,..> (integer and bool template arguments are all these kernels have)"""
  out = {}
  for n in names:
    m = re.match(r"_ZN4mcba(\d+)", n)
    if not m:
      out[n] = n
      continue
    k = int(m.group(1))
    base, rest = n[m.end():m.end() + k], n[m.end() + k:]
    m2 = re.match(r"(\d+)k_", rest)   # (a nested namespace, mcba::pnp::k_view_pose: the kernel's own name is the next component)
    if m2:
      k = int(m2.group(1))
      base, rest = rest[m2.end(1):m2.end(1) + k], rest[m2.end(1) + k:]
    args = re.findall(r"L[ibjm](\d+)E", rest.split("EEv")[0]) if rest.startswith("I") else []
    out[n] = base + ("<" + ",".join(args) + ">" if args else "")
  return out


def operands(line):
  op, _, rest = line.partition(" ")
  return op, [x.strip() for x in rest.split(",")] if rest else []


def classify(a, b):
  (opa, xa), (opb, xb) = operands(a), operands(b)
  if opa == opb and len(xa) == len(xb) and xa[:1] == xb[:1] and sorted(xa[1:]) == sorted(xb[1:]):
    return "commuted"
  base = lambda op: re.sub(r"_(i32|u32|i64|u64)$", "", op)
  for p, q in INVERSE:
    if {base(opa), base(opb)} == {p, q}:
      return "inverted"
  return "other"


def differing(a, b):
  kinds = {"commuted": 0, "inverted": 0, "other": 0}
  for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
    if tag == "equal":
      continue
    if tag == "replace" and i1 - i0 == j1 - j0:
      for x, y in zip(a[i0:i1], b[j0:j1]):
        kinds[classify(x, y)] += 1
    else:
      kinds["other"] += max(i1 - i0, j1 - j0)
  return kinds


def kernel_descriptors(lib):
  """sorted *.kd symbols of every gfx950 code object embedded in a libmcba.so (the AMDGPU ELF images inside .hip_fatbin)"""
  import struct
  data, out, pos = open(lib, "rb").read(), [], 1
  while True:
    pos = data.find(b"\x7fELF\x02\x01", pos)
    if pos < 0:
      return sorted(out)
    if struct.unpack_from("<H", data, pos + 18)[0] == 224:   # EM_AMDGPU
      shoff, = struct.unpack_from("<Q", data, pos + 40)
      shentsize, shnum = struct.unpack_from("<HH", data, pos + 58)
      sec = [struct.unpack_from("<IIQQQQIIQQ", data, pos + shoff + i * shentsize) for i in range(shnum)]
      for typ, off, size, link, entsize in [(x[1], x[4], x[5], x[6], x[9]) for x in sec]:
        if typ == 2:   # SHT_SYMTAB
          stroff = sec[link][4]
          for i in range(size // entsize):
            name_off, = struct.unpack_from("<I", data, pos + off + i * entsize)
            end = data.index(b"\0", pos + stroff + name_off)
            name = data[pos + stroff + name_off:end].decode()
            if name.endswith(".kd"):
              out.append(name)
    pos += 4


def main():
  if sys.argv[1] == "--kd":   # (a): the kernels of two built libraries
    ka, kb = kernel_descriptors(sys.argv[2]), kernel_descriptors(sys.argv[3])
    print(f"kernel descriptor symbols (*.kd) in the gfx950 code objects: A {len(ka)}, B {len(kb)}, lists identical: {ka == kb}")
    for n in sorted(set(ka) ^ set(kb)):
      print(f"  only in {'A' if n in ka else 'B'}: {n}")
    return
  a_dir, a_log, b_dir, b_log = sys.argv[1:5]
  prefixes = sys.argv[5:]
  ua, ub = kernels_of(a_dir), kernels_of(b_dir)
  ka, kb = set(ua), set(ub)
  print(f"kernel descriptors: A {len(ka)}, B {len(kb)}, only in A {len(ka - kb)}, only in B {len(kb - ka)}")
  for n in sorted(ka ^ kb):
    print(f"  only in {'A' if n in ka else 'B'}: {' '.join(sorted((ua if n in ka else ub)[n]))} {n}")
  la, lb = listings(a_dir), listings(b_dir)
  ra, rb = resources(a_log), resources(b_log)
  names = demangle(sorted(ka | kb))
  moved = sorted(n for n in ka & kb if sorted(ua[n]) != sorted(ub[n]))
  print(f"kernels emitted by other translation units in B than in A: {len(moved)}")
  for n in moved:
    print(f"  {names[n]}: {' '.join(sorted(ua[n]))} -> {' '.join(sorted(ub[n]))}")
  print("kernel [unit] | " + " ".join(SHORT) + " (A, '-> B' where it differs) | instructions A B | differing lines: commuted inverted other")
  same = changed = 0
  fam = {}   # kernel family -> [instantiations, identical listing and figures]
  for n in sorted(ka & kb, key=lambda k: names[k]):
    # (a symbol that several units emit has one listing per unit: compared as sets, the first of each printed)
    sa, sb = sorted(set(map(tuple, la.get(n, {}).values()))), sorted(set(map(tuple, lb.get(n, {}).values())))
    a, b = list(sa[0]) if sa else [], list(sb[0]) if sb else []
    unit = " ".join(sorted(ub[n]))
    if sa == sb:
      same += 1
    else:
      changed += 1
    # the remarks of a symbol come once per translation unit that emits it, in build order; figures of a symbol that differ
    # between units are all printed
    fa = sorted({tuple(r.get(f, "?") for f in FIELDS) for r in ra.get(n, [{}])})
    fb = sorted({tuple(r.get(f, "?") for f in FIELDS) for r in rb.get(n, [{}])})
    f = fam.setdefault(names[n].split("<")[0], [0, 0])
    f[0] += 1
    if sa == sb and fa == fb:   # identical kernels are only counted, per family below
      f[1] += 1
      continue
    fig = " ".join(x if x == y else f"{x}->{y}" for x, y in zip(fa[0], fb[0])) if len(fa) == len(fb) == 1 else f"{fa} | {fb}"
    k = differing(a, b)
    print(f"{names[n]} [{unit}] | {fig} | {len(a)} {len(b)} | {k['commuted']} {k['inverted']} {k['other']}")
  print(f"kernels with identical listings: {same}; with differing lines: {changed}")
  print("family: instantiations, of them with identical listing and figures")
  for name in sorted(fam):
    if not prefixes or any(name.startswith(p) for p in prefixes) or fam[name][0] != fam[name][1]:
      print(f"  {name}: {fam[name][0]} {fam[name][1]}")

if __name__ == "__main__":
  main()
