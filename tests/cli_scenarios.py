"""The command line's transcripts: scenarios, the normaliser, and the runner shared by
tests/test_cli_transcripts.py (which compares raft-tla_amd/rtla with tests/golden/cli/) and
tests/golden/make_cli_golden.py (which writes those fixtures from another build's binary).

A scenario builds its files under a fresh directory and returns the command lines to run there, in order; a
transcript is, per command, the exit code and the normalised stdout and stderr."""
import collections
import os
import re
import shutil
import subprocess

from cli_util import ROOT, model_dir

GOLDEN = os.path.join(ROOT, "tests", "golden", "cli")
# expect: words that the last command's output must hold, so that a scenario tests what its name says
Scenario = collections.namedtuple("Scenario", "name gpu build mask_states sort_ranks expect",
                                  defaults=(0, False, ""))
SCENARIOS = []

# ---- normalisation: only what two runs of one binary differ in (tests/golden/cli/EVIDENCE.md records, for the
# three beyond clock, rate, device and directory, which runs differed where).  A pattern keeps the words around.
MASKS = [
    (re.compile(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d"), "<TIME>"),                    # now_str()
    (re.compile(r"Finished in [0-9.]+s"), "Finished in <S>s"),
    (re.compile(r"[0-9.]+ ms\b"), "<MS> ms"),                                      # level / audit kernel times
    (re.compile(r"[0-9.]+ s on the GPU"), "<S> s on the GPU"),                     # the walks' kernel time
    (re.compile(r"\([0-9.e+a-z]+ (d?s)/min\)"), r"(<RATE> \1/min)"),               # Progress: states per minute
    (re.compile(r"[0-9.e+a-z]+ (steps|generated)/s"), r"<RATE> \1/s"),             # Simulation: per second
    (re.compile(r"(on 1 GPU: ).*"), r"\1<DEVICE>"),                                # rtla_device_info
]
# -coverage: which action is credited with a distinct state that two reach in one level depends on timing (the
# count of generated states per action does not, and stays compared)
COVERAGE = (re.compile(r"( of module raft>: )\d+(:\d+)"), r"\1<DISTINCT>\2")
# a trace block, its label and its variables: the search keeps for a state the parent that inserted it first, so
# which of several shortest behaviours is printed depends on timing; the number of blocks does not, nor does
# State 1 (the initial state), nor what follows the search's part of the trace (a walk's steps, fixed by the seed)
STATE_BODY = re.compile(r"^State (\d+): <.*>\n(?:.+\n)*", re.M)
RANK_LINE = re.compile(r"^rtla rank \d+ of \d+ ready")


def normalise(text, tmp, mask_states=0, sort_ranks=False, strict=False):
    """mask_states: the bodies of State 2 .. State mask_states are masked; strict: the masks of MASKS alone, to
    find out what else differs between runs."""
    text = text.replace(tmp, "<TMP>")
    for pat, sub in MASKS if strict else MASKS + [COVERAGE]:
        text = pat.sub(sub, text)
    if mask_states and not strict:
        text = STATE_BODY.sub(lambda m: "State %s: <STATE>\n" % m.group(1)
                              if 2 <= int(m.group(1)) <= mask_states else m.group(0), text)
    lines = text.split("\n")
    if sort_ranks and not strict:  # the ranks of a -gpus run write stderr side by side: their lines have no order
        ranks = [i for i, line in enumerate(lines) if RANK_LINE.match(line)]
        for i, line in zip(ranks, sorted(lines[i] for i in ranks)):
            lines[i] = line
    return lines


def transcript(cli, scenario, tmp, timeout=300, strict=False):
    """Run the scenario's commands with the binary `cli`; one record per command."""
    tmp = str(tmp)
    out = []
    for args, env in scenario.build(tmp):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=timeout, env=e)
        out.append({"args": [a.replace(tmp, "<TMP>") for a in args], "returncode": r.returncode,
                    "stdout": normalise(r.stdout, tmp, scenario.mask_states, strict=strict),
                    "stderr": normalise(r.stderr, tmp, sort_ranks=scenario.sort_ranks, strict=strict)})
    return out


def golden_path(name):
    return os.path.join(GOLDEN, name + ".json")


# ---- scenario building blocks
SKIP = ["-skip-spec-check"]
SMALL = SKIP + ["-fpbits", "18", "-membudget", str(1 << 28)]
PRED22 = SKIP + ["-fpbits", "22", "-membudget", str(1 << 30)]  # the three-server shape (tests/test_pred_cli.py)
N2T2 = (2, 1, 2, 1, 1, 1)
N2T3 = (2, 1, 3, 1, 1, 1)
N3T3 = (3, 1, 3, 1, 1, 1)
STATE_DEFS = """NoTwoLeadersAgain == \\A i, j \\in Server :
    (state[i] = Leader /\\ state[j] = Leader) => i = j

NoLeader == ~ \\E i \\in Server : state[i] = Leader

TermsFromOne == \\A i \\in Server : currentTerm[i] >= 1

"""


def spec_file(tmp, name):
    """A copy of specs/<name> under tmp, so that every path the program prints starts with tmp."""
    os.makedirs(os.path.join(tmp, "specs"), exist_ok=True)
    return shutil.copy(os.path.join(ROOT, "specs", name), os.path.join(tmp, "specs", name))


def both_kinds(tmp):
    """specs/MCActions.tla's action definitions and three state definitions in one file."""
    text = open(os.path.join(ROOT, "specs", "MCActions.tla")).read()
    at = text.index("\\* ---- laws")
    path = os.path.join(tmp, "Both.tla")
    open(path, "w").write(text[:at] + STATE_DEFS + text[at:])
    return path


def written(tmp, name, text):
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, name)
    open(path, "w").write(text)
    return path


def scenario(name, **flags):
    def add(build):
        SCENARIOS.append(Scenario(name, flags.pop("gpu", False), build, **flags))
        return build
    return add


def simple(name, shape, invariants, args, gpu=False, pred=None, extra="", edit=None, **model):
    """One command over model_dir's MC.tla / MC.cfg: `args` + [-predicates pred] -config cfg spec.  pred: a file
    of specs/, a callable making one under tmp, or a path relative to tmp; edit: rewrites the cfg's text."""
    def build(tmp):
        spec, cfg = model_dir(tmp, *shape, list(invariants), extra=extra, **model)
        if edit:
            text = open(cfg).read()
            assert edit(text) != text, name
            open(cfg, "w").write(edit(text))
        a = list(args)
        if pred:
            a += ["-predicates", pred(tmp) if callable(pred) else
                  spec_file(tmp, pred) if pred.startswith("MC") else os.path.join(tmp, pred)]
        return [(a + ["-config", cfg, spec], {})]
    SCENARIOS.append(Scenario(name, gpu, build))


# ---- no device needed: usage and refusals, in the order main reaches them
for _name, _args in [("usage", []), ("help", ["-h"]), ("unknown_option", ["-frobnicate", "1", "x.tla"]),
                     ("option_without_value", ["x.tla", "-config"]), ("gpus_0", ["-gpus", "0", "x.tla"]),
                     ("simulate_unknown_option", ["-simulate", "num=3,walks=4", "x.tla"]),
                     ("simulate_gpus_2", ["-simulate", "-gpus", "2", "x.tla"]),
                     ("audit_gpus_2", SKIP + ["-audit", "LogMatching", "-gpus", "2", "x.tla"]),
                     ("audit_simulate", SKIP + ["-audit", "LogMatching", "-simulate", "x.tla"]),
                     ("audit_no_names", ["-audit", ",", "x.tla"]),
                     ("predicates_gpus_2", ["-gpus", "2", "-predicates", "p.tla", "x.tla"]),
                     ("audit_bfs_levels_0", ["-audit", "LogMatching", "-bfs-levels", "0", "x.tla"]),
                     ("depth_70000", ["-simulate", "-depth", "70000", "-seed", "1", "x.tla"]),
                     ("no_spec", ["-config", "x.cfg"]),
                     ("missing_spec", ["-config", "x.cfg", "nowhere/x.tla"])]:
    SCENARIOS.append(Scenario(_name, False, lambda tmp, a=_args: [(a, {})]))
SCENARIOS.append(Scenario("gpus_2_dry_run", False,
                          lambda tmp: [(["-gpus", "2", "-config", "x.cfg", "x.tla"], {"RTLA_CLI_DRYRUN": "1"})],
                          sort_ranks=True))
SCENARIOS.append(Scenario("rank_outside_world", False,
                          lambda tmp: [(["-gpus", "2", "x.tla"], {"RTLA_RANK": "3", "RTLA_WORLD": "2"})]))


@scenario("modified_spec")
def _(tmp):
    written(tmp, "raft.tla", "---- MODULE raft ----\nEXTENDS Naturals\nVARIABLE x\n====\n")
    cfg = written(tmp, "raft.cfg", "SPECIFICATION Spec\nINVARIANT NoTwoLeaders\n")
    return [(["-config", cfg, os.path.join(tmp, "raft.tla")], {})]


@scenario("wrapper_without_raft")
def _(tmp):
    spec, cfg = model_dir(tmp, *N2T2, ["NoTwoLeaders"])
    return [(["-config", cfg, spec], {})]


@scenario("missing_cfg")
def _(tmp):
    spec, cfg = model_dir(tmp, *N2T2, ["NoTwoLeaders"])
    return [(SKIP + ["-config", os.path.join(tmp, "Other.cfg"), spec], {})]


@scenario("builtin_names_on_raft_itself")
def _(tmp):
    spec, cfg = model_dir(tmp, *N2T2, ["StateMachineSafety", "LeaderCompleteness"])
    raft = written(tmp, "raft.tla", open(spec).read().replace("MODULE MC", "MODULE raft"))
    return [(SKIP + ["-config", cfg, raft], {})]


simple("no_constraint", N2T2, ["NoTwoLeaders"], SKIP, constraint=False)
simple("unknown_invariant", N2T2, ["TypeOK"], SKIP)
simple("invariant_state_constraint", N2T2, ["StateConstraint"], SKIP)
simple("unknown_symmetry", N2T2, ["NoTwoLeaders"], SKIP, extra="SYMMETRY Other\n")
simple("missing_max_term", N2T2, ["NoTwoLeaders"], SKIP, edit=lambda t: t.replace("    MaxTerm = 2\n", ""))
simple("missing_server_set", N2T2, ["NoTwoLeaders"], SKIP, edit=lambda t: t.replace("Server = {r1, r2}", ""))
simple("wrong_string_constant", N2T2, ["NoTwoLeaders"], SKIP,
       edit=lambda t: t.replace('Leader = "Leader"', 'Leader = "Boss"'))
simple("cfg_view", N2T2, ["NoTwoLeaders"], SKIP, extra="VIEW vars\n")
simple("cfg_bad_constant", N2T2, ["NoTwoLeaders"], SKIP, extra="CONSTANT Extra =")
simple("cfg_unexpected_token", N2T2, ["NoTwoLeaders"], SKIP, edit=lambda t: "stray\n" + t)
simple("specification_other", N2T2, ["NoTwoLeaders"], SKIP, edit=lambda t: t.replace("Spec\n", "LiveSpec\n", 1))
simple("audit_unknown_name", N2T2, ["ElectionSafety"], SKIP + ["-audit", "TypeOK"])
simple("audit_known_then_unknown", N2T2, ["ElectionSafety"], SKIP + ["-audit", "StateMachineSafety,TypeOK"])
# -predicates: user INVARIANTs
simple("user_invariant_without_file", N2T2, ["PNoTwoLeaders"], SKIP)
simple("user_invariant_not_in_file", N2T2, ["NoSuchThing"], SKIP, pred="MCPredicates.tla")
simple("action_named_as_invariant", N2T2, ["LeadersStay"], SKIP, pred="MCActions.tla")
simple("type_error_in_named_definition", N2T2, ["PNoTwoLeaders"], SKIP,
       pred=lambda tmp: written(tmp, "bad.tla", "PNoTwoLeaders == \\A i \\in Server :\n  state[i] = 1\n"))
simple("type_error_in_unnamed_definition", N2T2, ["Fine"], SKIP,
       pred=lambda tmp: written(tmp, "bad.tla", "Fine == \\A i \\in Server : currentTerm[i] >= 1\n\n"
                                "Unnamed == \\A i \\in Server :\n  state[i] = 1\n"))
simple("missing_file_invariant", N2T2, ["PNoTwoLeaders"], SKIP, pred="nowhere.tla")
# PROPERTY
simple("property_without_file", N2T2, [], SKIP, extra="PROPERTY LeadersStay\n")
simple("property_unknown_name", N2T2, [], SKIP, pred="MCActions.tla", extra="PROPERTY NoSuchAction\n")
simple("property_state_definition", N2T2, [], SKIP, pred="MCPredicates.tla", extra="PROPERTIES LeadersStay NoCommit\n")
simple("property_missing_file", N2T2, [], SKIP, pred="nowhere.tla", extra="PROPERTY LeadersStay\n")
simple("property_prime_on_bound_name", N2T2, [], SKIP, extra="PROPERTY Frozen\n",
       pred=lambda tmp: written(tmp, "bad.tla", "Frozen == [][ \\A i \\in Server :\n  i' = i ]_vars\n"))
# CONSTRAINT
CONS = dict(constraint=False)
simple("constraint_without_file", N2T3, ["NoTwoLeaders"], SKIP, extra="CONSTRAINT StateConstraint OneCandidate\n", **CONS)
simple("constraint_not_in_file", N2T3, ["NoTwoLeaders"], SKIP, pred="MCConstraints.tla",
       extra="CONSTRAINT StateConstraint NoSuchThing\n", **CONS)
simple("constraint_missing_file", N2T3, ["NoTwoLeaders"], SKIP, pred="nowhere.tla",
       extra="CONSTRAINT StateConstraint OneCandidate\n", **CONS)
simple("constraint_without_state_constraint", N2T3, ["NoTwoLeaders"], SKIP, pred="MCConstraints.tla",
       extra="CONSTRAINT OneCandidate\n", **CONS)
simple("constraint_action_definition", N2T3, ["NoTwoLeaders"], SKIP, pred="MCActions.tla",
       extra="CONSTRAINT StateConstraint TermsNeverDecrease\n", **CONS)
simple("action_constraint", N2T3, ["NoTwoLeaders"], SKIP, pred="MCConstraints.tla",
       extra="CONSTRAINT StateConstraint\nACTION_CONSTRAINT OneCandidate\n", **CONS)
simple("constraint_with_simulate", N2T3, ["NoTwoLeaders"], SKIP + ["-simulate", "num=10", "-seed", "1"],
       pred="MCConstraints.tla", extra="CONSTRAINT StateConstraint OneCandidate\n", **CONS)
simple("constraint_type_error", N2T3, ["NoTwoLeaders"], SKIP, extra="CONSTRAINT StateConstraint OneCandidate\n",
       pred=lambda tmp: written(tmp, "bad.tla", "OneCandidate == \\A i \\in Server :\n  state[i] = 1\n"), **CONS)
# two rules broken at once: the first in main's order is the one reported
simple("order_property_before_invariant", N2T2, ["TypeOK"], SKIP, extra="PROPERTY NoSuchAction\n")
simple("order_constraint_name_before_no_state_constraint", N2T3, ["NoTwoLeaders"], SKIP, pred="MCConstraints.tla",
       extra="CONSTRAINT NoSuchThing\n", **CONS)
simple("order_symmetry_before_constants", N2T2, ["NoTwoLeaders"], SKIP, extra="SYMMETRY Other\n",
       edit=lambda t: t.replace("    MaxTerm = 2\n", ""))
simple("order_audit_name_before_constraint_name", N2T3, ["NoTwoLeaders"], SKIP + ["-audit", "TypeOK"],
       extra="CONSTRAINT StateConstraint NoSuchThing\n", **CONS)

# ---- on the GPU: each a search of a few seconds at most
G = dict(gpu=True)
simple("search_coverage_dump_levels", N2T2, ["NoTwoLeaders", "ElectionSafety"],
       SMALL + ["-coverage", "1", "-dump-levels", "-seed", "1"], **G)
simple("search_symmetry", N2T2, ["NoTwoLeaders"], SMALL + ["-seed", "1"], symmetry=True, **G)
simple("user_invariant_holds", N2T2, ["NoTwoLeaders", "MessagesWithinSenderTerm"], SMALL + ["-seed", "1"],
       pred="MCPredicates.tla", **G)
simple("user_invariant_violated", N2T3, ["NoTwoLeaders", "NobodyCommits"], SMALL + ["-seed", "1"],
       pred="MCConstraints.tla", **G)
simple("builtin_invariant_violated", N3T3, ["NoTwoLeaders"], PRED22 + ["-seed", "1"], **G)
simple("property_holds", N2T2, ["NoTwoLeaders"], SMALL + ["-seed", "1"], pred="MCActions.tla",
       extra="PROPERTIES LeaderAppendOnly TermsNeverDecrease\n", **G)
simple("property_violated", N2T2, [], SMALL + ["-seed", "1"], pred="MCActions.tla", extra="PROPERTY LeadersStay\n", **G)
simple("one_constraint", N2T3, ["NoTwoLeaders"], SMALL + ["-seed", "1"], pred="MCConstraints.tla",
       extra="CONSTRAINT StateConstraint OneCandidate\n", **G, **CONS)
simple("two_constraints", (2, 1, 3, 1, 1, 2), ["NoTwoLeaders"], SMALL + ["-seed", "1"], pred="MCConstraints.tla",
       extra="CONSTRAINTS StateConstraint TermsUpTo2 InFlightUpTo1\n", **G, **CONS)
simple("constraint_and_violated_user_invariant", N2T3, ["NoTwoLeaders", "NobodyCommits"], SMALL + ["-seed", "1"],
       pred="MCConstraints.tla", extra="CONSTRAINT StateConstraint OneCandidate\n", **G, **CONS)
AUDIT10 = SMALL + ["-seed", "1", "-bfs-levels", "10", "-audit"]
simple("audit_builtins", N2T2, ["ElectionSafety"], AUDIT10 + ["StateMachineSafety,LeaderCompleteness,NoTwoLeaders"], **G)
simple("audit_builtins_and_states", N2T2, ["ElectionSafety"], AUDIT10 + ["NoTwoLeaders,TermsFromOne,NoTwoLeadersAgain"],
       pred=both_kinds, **G)
simple("audit_actions", N2T2, [], AUDIT10 + ["LeaderAppendOnly,LeadersStay,NoTwoLeaders"], pred="MCActions.tla", **G)
simple("audit_all_action_violated", N2T2, [], AUDIT10 + ["NoTwoLeaders,TermsFromOne,LeadersStay,LeaderAppendOnly"],
       pred=both_kinds, **G)
simple("audit_all_state_violated", N2T2, [], AUDIT10 + ["NoTwoLeaders,NoLeader,TermsFromOne,LeaderAppendOnly"],
       pred=both_kinds, **G)
simple("audit_all_state_and_action_violated", N2T2, [], AUDIT10 + ["LogMatching,NoLeader,LeadersStay"],
       pred=both_kinds, **G)
simple("audit_all_builtin_and_action_violated", N3T3, ["ElectionSafety"],
       PRED22 + ["-seed", "1", "-bfs-levels", "19", "-audit", "NoTwoLeaders,TermsFromOne,LeadersStay"],
       pred=both_kinds, **G)
simple("audit_exhausted_search", N2T2, ["NoTwoLeaders"],
       SMALL + ["-seed", "1", "-bfs-levels", "100", "-audit", "StateMachineSafety"], **G)
SIM = ["-depth", "20", "-seed", "7", "-bfs-levels", "3"]
simple("simulate_plain", N2T2, ["NoTwoLeaders"], SMALL + ["-simulate", "num=2000"] + SIM, **G)
simple("simulate_sets_hold", N2T2, ["NoTwoLeaders", "NoTwoLeadersAgain"], SMALL + ["-simulate", "num=2000"] + SIM,
       pred=both_kinds, extra="PROPERTY LeaderAppendOnly\n", **G)
simple("simulate_action_violated", N2T2, ["NoTwoLeaders"], SMALL + ["-simulate", "num=2000"] + SIM,
       pred="MCActions.tla", extra="PROPERTY LeadersStay\n", **G)
simple("simulate_num_first", N2T2, ["NoTwoLeaders"], SMALL + ["-simulate", "num=500,first=1000"] + SIM, **G)


@scenario("checkpoint_then_recover", gpu=True)
def _(tmp):
    spec, cfg = model_dir(tmp, *N2T2, ["NoTwoLeaders"])
    prefix = os.path.join(tmp, "states", "ckpt")
    return [(SMALL + ["-seed", "1", "-checkpoint", "0.000001", "-checkpointdir", prefix, "-config", cfg, spec], {}),
            (SMALL + ["-seed", "1", "-recover", prefix, "-config", cfg, spec], {}),
            (SMALL + ["-seed", "1", "-recover", os.path.join(tmp, "states", "none"), "-config", cfg, spec], {})]


UNDEFINED = "The %s specified in the configuration file is not defined"
VIOLATED = "Error: %s is violated.\n"
# What the last command of a scenario must say (a golden that holds another refusal would pin the wrong thing),
# and the scenarios that print a trace: the one place that says whose State blocks are masked (STATE_BODY).
EXPECT = {
    "usage": "usage: rtla", "help": "usage: rtla", "option_without_value": "usage: rtla", "no_spec": "usage: rtla",
    "unknown_option": "unsupported option -frobnicate", "gpus_0": "usage: rtla",
    "simulate_unknown_option": "-simulate: unknown option walks=4", "simulate_gpus_2": "-simulate runs on one GPU",
    "audit_gpus_2": "-audit names at least one invariant", "audit_simulate": "-audit names at least one invariant",
    "audit_no_names": "-audit names at least one invariant", "predicates_gpus_2": "-predicates checks user-defined",
    "audit_bfs_levels_0": "-bfs-levels must be at least 1", "depth_70000": "-depth must be 0..65535",
    "missing_spec": "cannot read nowhere/x.tla", "gpus_2_dry_run": "rtla rank 1 of 2 ready",
    "rank_outside_world": "rank 3 of 2 does not match -gpus 2", "modified_spec": "has sha256",
    "wrapper_without_raft": "EXTENDS raft but", "missing_cfg": "cannot read config",
    "builtin_names_on_raft_itself": UNDEFINED % "invariant StateMachineSafety",
    "no_constraint": "no CONSTRAINT", "unknown_invariant": UNDEFINED % "invariant TypeOK",
    "invariant_state_constraint": UNDEFINED % "invariant StateConstraint",
    "unknown_symmetry": UNDEFINED % "symmetry Other", "missing_max_term": "constant MaxTerm is not assigned in",
    "missing_server_set": "constant Server is not assigned a set in",
    "wrong_string_constant": 'constant Leader must be bound to "Leader"', "cfg_view": "VIEW is not supported",
    "cfg_bad_constant": "bad CONSTANT near 'Extra'", "cfg_unexpected_token": "unexpected token 'stray'",
    "specification_other": "SPECIFICATION LiveSpec: only Spec", "audit_unknown_name": UNDEFINED % "invariant TypeOK",
    "audit_known_then_unknown": UNDEFINED % "invariant TypeOK",
    "user_invariant_without_file": UNDEFINED % "invariant PNoTwoLeaders",
    "user_invariant_not_in_file": UNDEFINED % "invariant NoSuchThing",
    "action_named_as_invariant": UNDEFINED % "invariant LeadersStay",
    "type_error_in_named_definition": "bad.tla:2:14: type error",
    "type_error_in_unnamed_definition": "bad.tla:4:14: type error",
    "missing_file_invariant": "cannot read the predicate file", "property_without_file": "MC.cfg: PROPERTY is not supported",
    "property_unknown_name": "MC.cfg: PROPERTY is not supported",
    "property_state_definition": "MC.cfg: PROPERTIES is not supported",
    "property_missing_file": "MC.cfg: PROPERTY is not supported",
    "property_prime_on_bound_name": "bad.tla:2:4: only a state variable may carry a prime",
    "constraint_without_file": UNDEFINED % "constraint OneCandidate",
    "constraint_not_in_file": UNDEFINED % "constraint NoSuchThing",
    "constraint_missing_file": UNDEFINED % "constraint OneCandidate",
    "constraint_without_state_constraint": "no CONSTRAINT",
    "constraint_action_definition": "The constraint TermsNeverDecrease is an action definition",
    "action_constraint": "ACTION_CONSTRAINT is not supported",
    "constraint_with_simulate": "-simulate with a user-defined CONSTRAINT (OneCandidate)",
    "constraint_type_error": "bad.tla:2:14: type error",
    "order_property_before_invariant": "MC.cfg: PROPERTY is not supported",
    "order_constraint_name_before_no_state_constraint": UNDEFINED % "constraint NoSuchThing",
    "order_symmetry_before_constants": UNDEFINED % "symmetry Other",
    "order_audit_name_before_constraint_name": UNDEFINED % "invariant TypeOK",
    "search_coverage_dump_levels": "<Timeout of module raft>: ", "search_symmetry": "Model checking completed.",
    "user_invariant_holds": "Model checking completed.", "property_holds": "Model checking completed.",
    "one_constraint": "Constraining the search by: OneCandidate.",
    "two_constraints": "Constraining the search by: TermsUpTo2, InFlightUpTo1.",
    "audit_builtins": "Audit completed.", "audit_builtins_and_states": "Invariant TermsFromOne holds in all",
    "audit_exhausted_search": "nothing to audit", "simulate_plain": "Simulation completed.",
    "simulate_sets_hold": "Checking in the walks: invariants NoTwoLeadersAgain; action properties LeaderAppendOnly.",
    "simulate_num_first": "(walk ids 1000..1499)", "checkpoint_then_recover": "cannot recover from",
}
TRACES = {
    "user_invariant_violated": VIOLATED % "Invariant NobodyCommits",
    "builtin_invariant_violated": VIOLATED % "Invariant NoTwoLeaders",
    "property_violated": VIOLATED % "Action property LeadersStay",
    "constraint_and_violated_user_invariant": VIOLATED % "Invariant NobodyCommits",
    "audit_actions": VIOLATED % "Action property LeadersStay",
    "audit_all_action_violated": VIOLATED % "Action property LeadersStay",
    "audit_all_state_violated": VIOLATED % "Invariant NoLeader",
    "audit_all_state_and_action_violated": VIOLATED % "Invariant NoLeader",
    "audit_all_builtin_and_action_violated": VIOLATED % "Invariant NoTwoLeaders",
    "simulate_action_violated": VIOLATED % "Action property LeadersStay",
}
SEARCH_PART = {"simulate_action_violated": 3}  # -bfs-levels 3: States 1..3 are the search's, the rest the walk's
SCENARIOS = [s._replace(expect=TRACES.get(s.name) or EXPECT.get(s.name, ""),
                        mask_states=SEARCH_PART.get(s.name, 1 << 30) if s.name in TRACES else 0) for s in SCENARIOS]
assert len({s.name for s in SCENARIOS}) == len(SCENARIOS)
assert all(s.expect for s in SCENARIOS)
