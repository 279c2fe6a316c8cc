#!/usr/bin/env python3
"""Static instruction histogram of the kernels of an assembly listing (hipcc --cuda-device-only -S).
    python tools/isa_sections.py file.s 'kernel-name-regex'     the first matching kernel, split at s_memtime markers (the CRT_POOL_STAMPS build) in layout order
    python tools/isa_sections.py --json file.s [regex]          every (matching) kernel of the file as one JSON object: demangled name -> the compiler's resource
                                                                metadata (vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size) and the
                                                                static instruction count by kind"""
import json, re, subprocess, sys

RESOURCES = ('vgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size')


def kind(t):
    if t.startswith('v_'): return 'valu'
    if t.startswith('ds_'): return 'lds'
    if t.startswith(('global_', 'buffer_', 'flat_', 'scratch_')): return 'vmem'
    if t.startswith(('s_load', 's_buffer_load')): return 'smem'
    if t.startswith(('s_cbranch', 's_branch')): return 'br'
    if t.startswith('s_waitcnt') or t == 's_nop': return 'wait'
    if t.startswith('s_'): return 'salu'
    return None


def bodies(lines, pat):
    """(mangled name, first line, line of s_endpgm) of every kernel whose name matches"""
    out = []; start = name = None
    for i, l in enumerate(lines):
        m = re.match(r'^(_Z\S+):', l)
        if start is None and m and pat.search(l): start, name = i, m.group(1)
        elif start is not None and l.strip().startswith('s_endpgm'): out.append((name, start, i)); start = None
    return out


def sections(lines):
    sec = []; cur = {}
    for l in lines:
        t = l.strip().split()[0] if l.strip() else ''
        if not t or t.startswith((';', '.')) or t.endswith(':'): continue
        if t == 's_memtime': sec.append(cur); cur = {}; continue
        k = kind(t)
        if k: cur[k] = cur.get(k, 0) + 1
    sec.append(cur)
    return sec


def metadata(lines):
    """mangled kernel name -> {resource: value} from the .amdgpu_metadata block: a kernel is an item at two spaces, its own keys stand at four"""
    out = {}; item = None
    def close():
        if item and '.name' in item: out[item['.name']] = {r: int(item['.' + r]) for r in RESOURCES}
    for l in lines:
        if l.startswith('  - .'): close(); item = {}; l = '    ' + l[4:]
        m = re.match(r'^    (\.\w+):\s*(\S+)$', l)
        if m and item is not None: item[m.group(1)] = m.group(2)
        if l.strip() == '.end_amdgpu_metadata': close(); item = None
    return out


def main():
    as_json = sys.argv[1] == '--json'
    args = sys.argv[2:] if as_json else sys.argv[1:]
    lines = open(args[0]).read().split('\n'); pat = re.compile(args[1] if len(args) > 1 else '')
    found = bodies(lines, pat)
    if not as_json:
        _, start, end = found[0]
        tot = {}
        for i, s in enumerate(sections(lines[start:end])):
            print(i, dict(sorted(s.items())), sum(s.values()))
            for k, v in s.items(): tot[k] = tot.get(k, 0) + v
        print('total', dict(sorted(tot.items())), sum(tot.values()))
        return
    meta = metadata(lines)
    names = [n for n, _, _ in found]
    pretty = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n') if names else []
    out = {}
    for (name, start, end), shown in zip(found, pretty):
        if name not in meta: continue                       # a device function, not a kernel
        tot = {}
        for s in sections(lines[start:end]):
            for k, v in s.items(): tot[k] = tot.get(k, 0) + v
        shown = re.sub(r'^void ', '', shown); shown = re.sub(r'\(.*$', '', shown)
        out[shown] = dict(meta[name], instructions=dict(sorted(tot.items())))
    json.dump(out, sys.stdout, indent=1); print()


if __name__ == '__main__':
    main()
