"""The search options of the seams (MCTS, SelfPlayManager, ModelEvaluator, train.py): which of them combine, and how an engine
is brought to a set of them.  A new option is wired into the seams here: its row(s) in CONFLICTS, its set / clear in apply_options.
The selection rule has a table and a function of its own (SELECTION_CONFLICTS, bring_selection): the seams call that function
on either side of apply_options.  So do candidate moves (CANDIDATE_CONFLICTS, bring_candidates), outermost: off before the
selection rule may come on, on after it has gone off."""

# Pairs of options that cannot be combined, with the text a seam refuses them with: the engine's table (g_conflicts in
# csrc/az_engine.hip) for the options the seams expose.  The first row whose two options are both on names the error.
CONFLICTS = (
    ("subtree_reuse", "virtual_loss", "subtree_reuse does not combine with virtual-loss batching"),
    ("evaluator", "subtree_reuse", "an external evaluator combines with neither subtree_reuse nor leaf_symmetry"),
    ("evaluator", "leaf_symmetry", "an external evaluator combines with neither subtree_reuse nor leaf_symmetry"),
    ("playout_cap", "subtree_reuse", "a playout cap combines with neither subtree_reuse nor an external evaluator"),
    ("playout_cap", "evaluator", "a playout cap combines with neither subtree_reuse nor an external evaluator"),
    ("forced_playouts", "subtree_reuse", "forced playouts do not combine with subtree_reuse"),
    ("gumbel", "subtree_reuse", "the Gumbel root search does not combine with subtree_reuse"),
    ("gumbel", "virtual_loss", "the Gumbel root search does not combine with virtual-loss batching"),
    ("gumbel", "forced_playouts", "the Gumbel root search does not combine with forced playouts"),
    ("gumbel", "evaluator", "the Gumbel root search needs the engine's own net: an outside evaluator returns priors, not logits"),
    ("solver", "subtree_reuse", "the solver does not combine with subtree_reuse"),
    ("solver", "virtual_loss", "the solver does not combine with virtual-loss batching"),
    ("solver", "forced_playouts", "the solver does not combine with forced playouts"),
    ("solver", "gumbel", "the solver does not combine with the Gumbel root search"),
    ("solver", "evaluator", "the solver needs the engine's own net: it does not combine with an outside evaluator"),
)
# ... and the options that need another one
NEEDS = (
    ("threat_search", "solver", "threat_search needs solver=True: it hands its results to the solver"),
)
# ... and the pairs the selection rule (az_set_selection) adds to the engine's table
SELECTION_CONFLICTS = (
    ("selection", "subtree_reuse", "the selection rule does not combine with subtree_reuse: a retained root has no fresh value"),
    ("selection", "solver", "the selection rule does not combine with the solver (and so not with the threat search)"),
    ("selection", "gumbel", "the selection rule does not combine with the Gumbel root search"),
)
# ... and the pairs candidate moves (az_set_candidates) add to it, read after SELECTION_CONFLICTS
CANDIDATE_CONFLICTS = (
    ("candidates", "subtree_reuse", "candidate moves do not combine with subtree_reuse: a retained root's priors were not made under the rule"),
    ("candidates", "gumbel", "candidate moves do not combine with the Gumbel root search: its top-m and target are defined over the legal cells"),
    ("candidates", "solver", "candidate moves do not combine with the solver (and so not with the threat search): no proof when moves were left out"),
    ("candidates", "selection", "candidate moves do not combine with the selection rule yet"),
    ("candidates", "evaluator", "candidate moves need the engine's own net: an outside evaluator returns priors, not logits"),
)


def switched_on(**options):
    """The names of the options that are on: virtual_loss other than 1; of the others whatever is neither None nor False."""
    return {name for name, v in options.items() if (v != 1 if name == "virtual_loss" else v is not None and v is not False)}


def check_combination(on, of=None):
    """ValueError for the first rule of CONFLICTS / NEEDS / SELECTION_CONFLICTS / CANDIDATE_CONFLICTS that the set `on` of option
    names breaks; of: only the rules that speak of this option."""
    for a, b, message in CONFLICTS:
        if a in on and b in on and of in (None, a, b):
            raise ValueError(message)
    for a, b, message in NEEDS:
        if a in on and b not in on and of in (None, a, b):
            raise ValueError(message)
    for a, b, message in SELECTION_CONFLICTS:
        if a in on and b in on and of in (None, a, b):
            raise ValueError(message)
    for a, b, message in CANDIDATE_CONFLICTS:
        if a in on and b in on and of in (None, a, b):
            raise ValueError(message)


def apply_options(eng, *, win_rule, start_positions, first, resign, playout_cap, forced_playouts, gumbel, solver, threat_search, rng=None):
    """Brings a new or cached engine to exactly these options (checked values as the seams keep them; None / False = off):
    each is set, or cleared if the engine still has it on.  Everything that goes off goes first, so that no option meets
    the left-overs of the last configuration in the engine's conflict table.  rng: "numpy" | "philox", the source of the engine's
    own tapes (az_set_rng; it meets no row of the table); None leaves the engine's mode alone."""
    if rng is not None and eng.rng() != rng:
        eng.set_rng(rng)
    if eng.win_rule() != win_rule:
        if eng.start_positions():
            eng.clear_start_positions()                   # they were validated under the other rule
        eng.set_win_rule(win_rule)
    if start_positions is None and eng.start_positions():
        eng.clear_start_positions()
    if resign is None and eng.resign()["threshold"]:
        eng.set_resign(0.0)
    if playout_cap is None and eng.playout_cap()["fast_sims"]:
        eng.set_playout_cap(0)
    if forced_playouts is None and eng.forced_playouts()["k"]:
        eng.set_forced_playouts(0.0)
    if gumbel is None and eng.gumbel()["m"]:
        eng.set_gumbel(0)
    if threat_search is None and eng.threat_search()[0]:
        eng.set_threat_search(0)                          # before the solver it needs may go
    if not solver and eng.solver():
        eng.set_solver(False)
    if start_positions is not None:
        eng.set_start_positions(*start_positions, first=first)      # by global game id, like the seed
    if resign is not None:
        eng.set_resign(**resign)
    if playout_cap is not None:
        # the engine's export filter does the selection: the packed records are the full plies' unless train_on_fast
        eng.set_playout_cap(playout_cap["fast_sims"], playout_cap["full"], export_full_only=not playout_cap["train_on_fast"])
    if forced_playouts is not None:
        eng.set_forced_playouts(forced_playouts["k"], forced_playouts["prune"])
    if gumbel is not None:
        eng.set_gumbel(min(gumbel["m"], eng.nn), gumbel["c_visit"], gumbel["c_scale"])     # a board has n * n cells
    if solver and not eng.solver():
        eng.set_solver(True)                              # before the threat search that needs it
    if threat_search is not None:
        eng.set_threat_search(**threat_search)
    return eng


def bring_selection(eng, selection, before):
    """The selection rule of a new or cached engine (selection: the checked dict, None = off), in two steps round apply_options
    and whatever else may switch one of its refused partners on: before=True takes it off unless the engine already has
    exactly this one, so that the solver, the Gumbel root search or subtree reuse never meet the last configuration's; before=
    False sets it once apply_options has switched those off."""
    have = eng.selection()
    same = selection is not None and have == dict(selection, on=True)
    if before:
        if have["on"] and not same:
            eng.set_selection(on=False)
    elif selection is not None and not same:
        eng.set_selection(**selection)
    return eng


def bring_candidates(eng, candidates, before):
    """Candidate moves of a new or cached engine (candidates: the checked dict, None = off), shaped like bring_selection and
    called outside it: before=True, ahead of everything that may switch a refused partner on (the selection rule included),
    takes the option off unless the engine already has exactly this radius; before=False, after everything that switches those
    off, sets it."""
    have = eng.candidates()
    same = candidates is not None and have == candidates["radius"]
    if before:
        if have and not same:
            eng.set_candidates(0)
    elif candidates is not None and not same:
        eng.set_candidates(candidates["radius"])
    return eng


def option_from_flags(error, flags, message):
    """A command line's flags for one option as the dict a seam takes.  flags: {key: value or None}, the option's own flag first.
    None without that one -- error(message) if any other was given --, else the values that were given."""
    given = {key: v for key, v in flags.items() if v is not None}
    if next(iter(flags)) not in given:
        if given:
            error(message)
        return None
    return given
