"""`--num_steps` / `--solver_order` / `--skip` of the CLIs that run on the edit-friendly DDPM noise space (`p2p/ --inversion_type ddpm`,
`ledits/`): 50 steps of the eta = 1 DDPM update by default, or N steps of the second-order multistep SDE-DPM-Solver++ (the solver
LEDITS++ is published with, meant for about 20 steps).  That 20 second-order steps edit as well as 50 first-order ones is the paper's
claim; the synthetic weights of this repository cannot show it, so 50 / order 1 stay the defaults."""
import argparse

NUM_STEPS = 50


class StoreGiven(argparse.Action):
    """store the value and note that the flag was given (`<dest>_given`): a default that depends on another flag is resolved later"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def add_solver_arguments(ap):
    ap.add_argument("--num_steps", type=int, default=NUM_STEPS, help="steps of inversion and edit (2 .. 1000)")
    ap.add_argument("--solver_order", type=int, default=1, choices=[1, 2],
                    help="1: the eta = 1 DDPM update; 2: second-order multistep SDE-DPM-Solver++ (LEDITS++'s solver, for about 20 "
                         "steps; its image quality at 20 steps is the paper's claim, not measured here)")


def check_solver_arguments(ap, args):
    if not 2 <= args.num_steps <= 1000:
        ap.error("--num_steps must lie in [2, 1000]")


def resolve_skip(args, fraction):
    """`--skip` as given; not given: the parser's default at NUM_STEPS steps (the paper's setting), int(fraction N) at any other N"""
    if getattr(args, "skip_given", False) or args.num_steps == NUM_STEPS:
        return args.skip
    return int(fraction * args.num_steps)
