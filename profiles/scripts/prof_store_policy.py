"""A/B of the store policy of the hand-off buffers (debug switch MCBA_STORE_THROUGH; 0 = plain stores everywhere).

    python profiles/scripts/prof_store_policy.py                       # switch on / off, every configuration, 3 rounds
    python profiles/scripts/prof_store_policy.py --configs cfg3 --policies on,records,assembly,off --rounds 5
    python profiles/scripts/prof_store_policy.py --lib old=/path/to/libmcba.so     # + a side-by-side older library

Policies: on = what ships (the switch left unset), off = MCBA_STORE_THROUGH=0, records / assembly = one site alone
(MCBA_STORE_THROUGH_SITES = 1 / 2: the records of k_linearize / the outputs of k_assemble).
Every (policy, round) is a process of its own (the switch is latched per process) and the policies ALTERNATE inside a round,
so that drift of the device shows up as spread inside a policy, not as a difference between them.  Per configuration:
  step        the evaluation step (k_prep + k_linearize + k_assemble + k_shared_final), 200 enqueued steps, best of 5, us
  k_linearize the dominant kernel alone by HIP events (mcba_time_linearize), us
  fused2 / gather3   the two launches of one LSMR iteration of the default solver by HIP events (mcba_time_lsmr_iteration), us
The summary prints min .. max over the rounds: a policy wins where its max is below the other's min.

For the kernel trace of the step run, in a run of its own (no counters in the same run):
    rocprofv3 --kernel-trace --stats -d OUT -- python bench.py --no-solve --no-cpu-baseline
"""
import argparse, json, os, subprocess, sys, time

POLICIES = {"on": [], "off": [("MCBA_STORE_THROUGH", "0")],
            "records": [("MCBA_STORE_THROUGH_SITES", "1")], "assembly": [("MCBA_STORE_THROUGH_SITES", "2")]}
CONFIGS = {"cfg3": 500, "cfg4": 1000, "cfg5_handeye": 400, "cfg2": 200}   # frames: the sizes BASELINE.md states


def child(configs, policy, switches):
  sys.path.insert(0, "."); sys.path.insert(0, "tests")
  from multical_amd import synthetic, calibration, _lib
  from multical_amd.backend import Handle
  if policy != "lib":                       # (a side-by-side library runs with whatever it does by default)
    for name, value in POLICIES[policy]:
      _lib.set_switch(name, value)
    for kv in filter(None, switches.split(",")):
      _lib.set_switch(*kv.split("=", 1))
  out = {}
  for cfg in configs:
    c = calibration.from_rig(synthetic.make_rig(cfg, frames=CONFIGS[cfg]))
    with Handle(c) as h:
      x0 = c.param_vec
      h.normal_equations(x0)
      tl = h.time_linearize(x0, 200)
      best = 1e9
      for rep in range(5):
        h.synchronize(); t0 = time.perf_counter()
        for k in range(200): h.normal_equations_device()
        h.synchronize(); best = min(best, (time.perf_counter() - t0) / 200)
      f2, g3 = h.time_lsmr_iteration(x0, 200)
      out[cfg] = dict(step=1e6 * best, k_linearize=1e3 * tl, fused2=1e3 * f2, gather3=1e3 * g3)
  print("RESULT" + json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--configs", default=",".join(CONFIGS))
  ap.add_argument("--policies", default="on,off", help="of " + " / ".join(POLICIES) + ", in the order they alternate")
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH",
                  help="another libmcba.so measured next to the policies (MCBA_LIB_PATH), with whatever it does by default")
  ap.add_argument("--switches", default="", help="other debug switches of every policy run, NAME=VALUE[,NAME=VALUE...]")
  ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
  a = ap.parse_args()
  configs = a.configs.split(",")
  if a.child is not None:
    return child(configs, a.child, a.switches)
  arms = [(p, p, None) for p in a.policies.split(",")] + [(l.split("=", 1)[0], "lib", l.split("=", 1)[1]) for l in a.lib]
  for _, policy, _ in arms:
    if policy != "lib" and policy not in POLICIES:
      ap.error("unknown policy " + policy)
  base = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_")}
  runs = {label: [] for label, _, _ in arms}
  for rnd in range(a.rounds):
    for label, policy, lib in arms:
      env = dict(base, MCBA_LIB_PATH=lib) if lib else base
      p = subprocess.run([sys.executable, os.path.abspath(__file__), "--configs", a.configs, "--switches", a.switches, "--child", policy], env=env,
                         capture_output=True, text=True, timeout=900)
      if p.returncode != 0:
        sys.exit("policy %s failed (rc %d):\n%s" % (label, p.returncode, p.stderr[-2000:]))
      r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][6:])
      runs[label].append(r)
      for cfg in configs:
        print("round %d  %-8s %-13s " % (rnd, label, cfg) + "  ".join("%s %7.2f" % kv for kv in r[cfg].items()), flush=True)
  print("\nmin .. max over %d rounds, us" % a.rounds)
  for cfg in configs:
    for label, _, _ in arms:
      cols = []
      for q in ("step", "k_linearize", "fused2", "gather3"):
        v = [r[cfg][q] for r in runs[label]]
        cols.append("%s %6.2f .. %6.2f" % (q, min(v), max(v)))
      print("%-13s %-8s " % (cfg, label) + "   ".join(cols))


if __name__ == "__main__":
  main()
