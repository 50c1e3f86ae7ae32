import re, sys, json, glob, os
D = sys.argv[1]
def grab(kind, v, r):
    return open(os.path.join(D, '%s_r%d_%s.txt' % (v, r, kind))).read()
cases = {}   # name -> {v: [values]}
def add(name, v, x): cases.setdefault(name, {'new': [], 'prev': []})[v].append(float(x))
rounds = sorted({int(re.search(r'_r(\d+)_', f).group(1)) for f in glob.glob(D + '/new_r*_index.txt')})
for r in rounds:
    for v in ('new', 'prev'):
        for m in re.finditer(r'Q =\s+(1|32)  stream  index.query\s+([\d.]+) us.*C call queued\s+([\d.]+) us', grab('index', v, r)):
            add('index  Q=%-2s index.query us' % m.group(1), v, m.group(2))
            add('index  Q=%-2s C call queued us' % m.group(1), v, m.group(3))
        for m in re.finditer(r'Q =\s+(\d+)  (no window|traverse 100 %|traverse   1 %)\s+rows per window\s+\S+\s+call\s+([\d.]+) us', grab('window', v, r)):
            add('window Q=%-2s %-14s C call us' % (m.group(1), m.group(2)), v, m.group(3))
        for m in re.finditer(r'd =  512  Q =\s+(\d+)  (resident, 1 % window|resident)\s+query\s+([\d.]+) us.*?C call\s+([\d.]+) us', grab('wide', v, r)):
            add('wide   Q=%-2s %-20s query us' % (m.group(1), m.group(2)), v, m.group(3))
            add('wide   Q=%-2s %-20s C call us' % (m.group(1), m.group(2)), v, m.group(4))
        add('bench.py --workload retrieval ms_per_step', v, json.loads(grab('bench', v, r).strip().splitlines()[-1])['ms_per_step'])
med = lambda x: sorted(x)[len(x) // 2]
print('%-50s %-26s %-26s %9s %9s  %s' % ('case', 'parent runs', 'new runs', 'parent md', 'new md', 'new median inside parent spread'))
bad = 0
for k, d in cases.items():
    lo, hi = min(d['prev']), max(d['prev'])
    ok = lo <= med(d['new']) <= hi
    faster = med(d['new']) < lo
    bad += not (ok or faster)
    print('%-50s %-26s %-26s %9.3f %9.3f  %s' % (k, ' '.join('%.1f' % x if x > 20 else '%.3f' % x for x in d['prev']), ' '.join('%.1f' % x if x > 20 else '%.3f' % x for x in d['new']),
          med(d['prev']), med(d['new']), 'yes' if ok else ('below it (faster)' if faster else 'NO: above it')))
print('cases above the parent spread: %d' % bad)
