"""The command-line flags of `--inversion_type npi` and proximal guidance, shared by the p2p/ and masactrl/ drivers (pure argparse: no
torch, no device).  `add_prox_arguments` declares them, `check_prox_arguments` turns a bad combination into an argparse error and
hands back the keyword arguments of `ProxGuidance.from_schedule` (None: no proximal guidance)."""

PROX_CHOICES = ("none", "l0", "l1")
XL_VERSIONS = ("xl-base", "smallxl")       # the `StableDiffusionXLPipeline` branch of `_bootstrap._build_pipe`


def add_prox_arguments(ap, default="none"):
    """default: what `--inversion_type npi` runs where --prox is not given ("none" on p2p, "l0" on masactrl, the folders the paper
    publishes on); every other inversion type runs without proximal guidance"""
    ap.add_argument("--prox", type=str, default=None, choices=PROX_CHOICES,
                    help=f"npi: proximal guidance, hard (l0) or soft (l1) thresholding of eps_c - eps_u (default with npi: {default})")
    ap.add_argument("--prox_quantile", type=float, default=0.7, help="npi: the per-row quantile of |eps_c - eps_u| the threshold is")
    ap.add_argument("--prox_steps", type=int, nargs=2, default=None, metavar=("A", "B"),
                    help="npi: threshold in the edit steps A <= i < B (default: all)")
    ap.add_argument("--recon_lr", type=float, default=1.0, help="npi: eta, the pull of x0 towards the encoded source outside the edit")
    ap.add_argument("--recon_t", type=int, default=400, help="npi: eta = --recon_lr at the timesteps below this, otherwise 0")
    ap.add_argument("--dilate_mask", type=int, default=1, help="npi: Chebyshev radius the edit mask is dilated by (0 .. 3)")
    ap.set_defaults(_prox_default=default)


def check_prox_arguments(ap, args, *, in_flight=1, nti_batch=1, blend=False, num_steps=50):
    """argparse errors of the flags above; -> None, or the keyword arguments of `ProxGuidance.from_schedule` past the timesteps"""
    npi = args.inversion_type == "npi"
    mode = args.prox if args.prox is not None else (args._prox_default if npi else "none")
    args.prox = mode
    if not 0.0 <= args.prox_quantile <= 1.0:
        ap.error(f"--prox_quantile is a quantile in [0, 1], got {args.prox_quantile}")
    if not 0 <= args.dilate_mask <= 3:
        ap.error(f"--dilate_mask is a radius in [0, 3], got {args.dilate_mask}")
    if npi and args.sd_version in XL_VERSIONS:
        ap.error("--inversion_type npi is built for the SD1.x / SD2.x pipelines, not for --sd_version " + args.sd_version)
    if npi and nti_batch > 1:
        ap.error("--nti_batch groups null-text optimisations; --inversion_type npi runs none (use --invert_batch / --in_flight)")
    if mode == "none":
        return None
    if not npi:
        ap.error(f"--prox {mode} is built on negative-prompt inversion: it needs --inversion_type npi, not {args.inversion_type}")
    if in_flight > 1:
        ap.error(f"--prox {mode} with --in_flight {in_flight}: proximal guidance runs one edit at a time (edit_many is out of scope)")
    if blend:
        ap.error(f"--prox {mode} with --blend_source_words / --blend_target_words: choose proximal guidance or a LocalBlend")
    if args.prox_steps is not None and not 0 <= args.prox_steps[0] <= args.prox_steps[1] <= num_steps:
        ap.error(f"--prox_steps A B must satisfy 0 <= A <= B <= {num_steps}")
    return dict(mode=mode, quantile=args.prox_quantile, radius=args.dilate_mask, prox_steps=args.prox_steps,
                recon_lr=args.recon_lr, recon_t=args.recon_t)
