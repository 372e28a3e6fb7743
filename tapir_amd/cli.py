"""tapir_compute.py, GPU edition: the reference's command line (bin/tapir_compute.py:18-53, 125-177) with the
per-locus HyPhy loop replaced by one batched call into the HIP engine.

Same positionals, same required/optional flags and defaults, same output directory contents
(Tree_<factor>_<depth>.newick, <alignment>.rates JSON per locus, phylogenetic-informativeness.sqlite).
`--hyphy` and `--template` are accepted for compatibility and ignored (there is no subprocess);
`--multiprocessing` parallelises the host side only (NEXUS parsing, .rates files).  New, opt-in flags only: --device, --exchangeabilities / --subs-model,
--integral-mode, --full-precision-rates, --gamma-categories / --gamma-alpha, --site-model, --rate-estimator,
--bootstrap / --bootstrap-seed / --bootstrap-level (site-bootstrap bands in a second file,
phylogenetic-informativeness-bootstrap.sqlite; the other outputs stay byte for byte the same), --quartets (quartet signal
and noise in another file of its own, phylogenetic-informativeness-quartets.sqlite; again nothing else changes),
--unequal-quartets / --tree-quartets (the same for quartets with four tip lengths of their own, typed or read off the input
tree's internodes, in phylogenetic-informativeness-unequal-quartets.sqlite), --exact-quartets / --exact-quartets-window (the
exact resolution probabilities beside the normal approximation: a table quartet_exact in those quartet files),
--locus-sets / --locus-sets-order / --locus-sets-max / --locus-sets-target (accumulation curves over an ordered list of loci:
tables locus_set, locus_set_summary and, with --exact-quartets, locus_set_exact in those quartet files),
--parametric-bootstrap / --parametric-bootstrap-seed / --parametric-bootstrap-level (the rates re-estimated on simulated
alignments: bands in phylogenetic-informativeness-parametric-bootstrap.sqlite, per-site moments in NAME.rates-bootstrap.json),
--posterior-pi / --posterior-pi-seed / --posterior-pi-level (with --rate-estimator eb: the posterior of the sites' rate
categories carried into the PI profile, analytic mean and sd and the band of the posterior draws in
phylogenetic-informativeness-posterior.sqlite; conditional on the fitted scale and shape; nothing else changes).

Several GPUs: launch it with `python -m torch.distributed.run --nproc-per-node G bin/tapir_compute.py ...` (one process
per GPU).  The files are dealt round-robin over the ranks (what `Pool.map(worker, params)` did over cores,
bin/tapir_compute.py:159-164); every rank writes the .rates files of its own loci into the one output directory
rank 0 created; the per-locus PI rows are collected with a single all-gather (tapir_amd/dist.py: RCCL, or gloo
without GPUs) and rank 0 writes the sqlite file in the original file order.

Stage 1 of the HyPhy script (203-model fit + model averaging of the GTR exchangeabilities,
models_and_rates.bf:405-897) runs on the GPU too (tapir_amd/stage1.py) unless the exchangeabilities are given
with --exchangeabilities / --subs-model, or a fixed model is chosen with --site-model jc / f81.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

from . import base, compute, db, newick, pipeline
from . import dist as tdist


LAST_TIMINGS = {}   # seconds per stage of the last main() call on this rank (tools/e2e_cli_timing.py)


def get_args(argv=None):
    """Get CLI arguments and options (mirrors bin/tapir_compute.py:18-53)."""
    parser = argparse.ArgumentParser(description="""tapir:  compute the
            phylogenetic informativeness of DNA loci""")
    parser.add_argument('alignments', help="The folder of alignments", action=base.FullPaths, type=base.is_dir)
    parser.add_argument('tree', help="The input tree", action=base.FullPaths)
    required = parser.add_argument_group("required arguments")
    required.add_argument('--times', help="""Comma-separated list of start
        times of interest (MYA)""", type=base.get_list_from_ints, required=True)
    required.add_argument('--intervals', help="""Comma-separated list of
        interval ranges of interest (i,e. in MYA)""", type=base.get_list_from_ranges, required=True)
    parser.add_argument('--tree-format', help="The format of the tree", dest='tree_format',
                        choices=['nexus', 'newick'], default='newick')
    parser.add_argument('--output', help="The path to the output directory", default=os.getcwd(),
                        action=base.FullPaths, type=base.is_dir)
    parser.add_argument('--hyphy', help="Ignored (kept for compatibility): there is no hyphy subprocess",
                        default="hyphy2")
    parser.add_argument('--template', help="Ignored (kept for compatibility)", default=None)
    parser.add_argument('--threshold', help="""Minimum number of taxa without
        a gap for a site to be considered informative""", default=3, type=int)
    parser.add_argument('--multiprocessing', help="""Enable parallel
        reading of alignments and writing of site-rate files (the rates themselves are always batched on the GPU)""",
                        default=False, action='store_true')
    parser.add_argument('--site-rates', default=False, action='store_true',
                        help="Use previously calculated site rates")
    parser.add_argument('--subset-pi-map-file', help="""Calculate PI for a
        subset of sites. If specified, this should be a tab-delimited file
        with the alignment file name in the 1st column, the start of the
        interval (0-offset) in the 2nd column, and the end of the interval in
        the 3rd column.""")
    new = parser.add_argument_group("MI355X engine options (not in the reference)")
    new.add_argument('--device', type=int, default=0, help="HIP device ordinal")
    new.add_argument('--exchangeabilities', type=_six_floats, default=None,
                     help="AC,AG,AT,CG,CT,GT used for every locus (default: model-averaged estimates per locus, "
                          "as the HyPhy script computes them)")
    new.add_argument('--subs-model', default=None,
                     help="tab-delimited file: alignment file name, AC, AG, AT, CG, CT, GT [, A, C, G, T frequencies]")
    new.add_argument('--integral-mode', choices=['quadpack', 'closed'], default='quadpack',
                     help="quadpack = emulate scipy.integrate.quad incl. its error column; closed = analytic")
    new.add_argument('--gamma-categories', type=int, default=1,
                     help="K > 1: discrete-gamma mixture of K rate categories on top of each site's rate (GTR+G; the "
                          "reference's HyPhy script has none, so K = 1 is the drop-in setting)")
    new.add_argument('--gamma-alpha', type=float, default=0.5, help="shape of that gamma distribution")
    new.add_argument('--reference-start', action='store_true',
                     help="start every site's optimiser at siteRate = 1 as the HyPhy script does (models_and_rates.bf:1050) "
                          "instead of at the site's parsimony rate: identical on unimodal sites, and on the rare multimodal "
                          "ones the optimum uphill of HyPhy's start; costs about one likelihood evaluation per site")
    new.add_argument('--full-precision-rates', action='store_true',
                     help="do not round site rates to 4 decimals before PI (the reference rounds through its JSON file)")
    new.add_argument('--site-model', choices=['locus', 'jc', 'f81'], default='locus',
                     help="locus = the locus' GTR model (stage-1 estimates, or --exchangeabilities / --subs-model); "
                          "jc = Jukes-Cantor (equal base frequencies, exchangeabilities 1; PhyDesign's other model); "
                          "f81 = exchangeabilities 1 with the locus' empirical base frequencies.  jc and f81 skip stage 1 "
                          "and run a closed-form site-rate kernel")
    new.add_argument('--rate-estimator', choices=['ml', 'eb'], default='ml',
                     help="ml = each site's maximum-likelihood rate (the reference's estimator); eb = empirical Bayes: the "
                          "posterior mean of the site's rate under a discrete-gamma prior whose scale and shape are fitted "
                          "to the locus (Yang 1994), so a site without a change gets a small positive rate instead of 0")
    new.add_argument('--eb-categories', type=int, default=None,
                     help="categories of the empirical-Bayes prior, 2..16 (default 8); needs --rate-estimator eb")
    new.add_argument('--eb-alpha', type=float, default=None,
                     help="fix the shape of the empirical-Bayes prior (default: estimated per locus); needs --rate-estimator eb")
    new.add_argument('--eb-alpha-bounds', type=_two_floats, default=None,
                     help="LO,HI: range in which the shape is estimated (default 0.2,50); needs --rate-estimator eb")
    new.add_argument('--bootstrap', type=int, default=0, metavar='B',
                     help="B in 2..4096: site bootstrap of every locus' PI profile and interval integrals with B resamples of "
                          "its columns (the fitted model held fixed); mean, sd and a confidence band per entry go into "
                          "phylogenetic-informativeness-bootstrap.sqlite.  0 = off")
    new.add_argument('--bootstrap-seed', type=int, default=None, help="seed of the resampling (default 1); needs --bootstrap")
    new.add_argument('--bootstrap-level', type=float, default=None,
                     help="coverage of the band [lo, hi], in (0, 1) (default 0.95); needs --bootstrap")
    new.add_argument('--parametric-bootstrap', type=int, default=0, metavar='B',
                     help="B in 2..4096: parametric bootstrap of the site rates: B times every column is simulated down the tree "
                          "under its locus' fitted model at its own fitted rate (the observed missing cells kept), its rate "
                          "re-estimated and the PI profile recomputed; mean, sd and a confidence band per entry go into "
                          "phylogenetic-informativeness-parametric-bootstrap.sqlite, mean and sd of every site's rate into "
                          "NAME.rates-bootstrap.json.  Not with --site-rates, --rate-estimator eb or --gamma-categories above 1.  "
                          "0 = off")
    new.add_argument('--parametric-bootstrap-seed', type=int, default=None,
                     help="seed of the simulation (default 1); needs --parametric-bootstrap")
    new.add_argument('--parametric-bootstrap-level', type=float, default=None,
                     help="coverage of the band [lo, hi], in (0, 1) (default 0.95); needs --parametric-bootstrap")
    new.add_argument('--posterior-pi', type=int, default=0, metavar='B',
                     help="B in 2..4096, with --rate-estimator eb: the posterior of every site's rate category carried into the "
                          "locus' PI profile and interval integrals -- their posterior mean and sd (analytic) and the band of B "
                          "posterior draws go into phylogenetic-informativeness-posterior.sqlite.  Conditional on the fitted "
                          "scale and shape, the model and the tree.  0 = off")
    new.add_argument('--posterior-pi-seed', type=int, default=None, help="seed of the draws (default 1); needs --posterior-pi")
    new.add_argument('--posterior-pi-level', type=float, default=None,
                     help="coverage of the band [lo, hi], in (0, 1) (default 0.95); needs --posterior-pi")
    new.add_argument('--quartets', type=_quartets, default=None, metavar='T:to[,T:to...]',
                     help="signal and noise of four-taxon trees ((a:T,b:T),(c:T,d:T)) with an internode of length to, both in "
                          "the tree's time units (floats; to > 0, T >= 0, T + to <= tree depth): per locus the expected numbers "
                          "of signal and noise sites and the probabilities that it resolves the internode correctly, "
                          "incorrectly or not at all (Townsend, Su & Tekle 2012) go into "
                          "phylogenetic-informativeness-quartets.sqlite.  With --site-rates it needs the loci's model: "
                          "--site-model jc|f81 or --exchangeabilities")
    new.add_argument('--unequal-quartets', type=_unequal_quartets, default=None, metavar='Ta/Tb/Tc/Td:to[,...]',
                     help="signal and noise of four-taxon trees ((a:Ta,b:Tb),(c:Tc,d:Td)) with four tip branches of their own "
                          "and an internode of length to, in the tree's time units (floats; to > 0, tips >= 0; at most 256): "
                          "per locus the expected numbers of signal sites and of noise sites for either wrong topology and the "
                          "probabilities of ab|cd, ac|bd, ad|bc or no resolution (Su & Townsend 2015) go into "
                          "phylogenetic-informativeness-unequal-quartets.sqlite.  The lengths are not held against the tree's "
                          "depth: a lineage through the parent of a node can be nearly twice as long.  Under --site-rates the "
                          "model rule of --quartets applies")
    new.add_argument('--tree-quartets', default=False, action='store_true',
                     help="the same for every internode of the input tree, each with the nearest tip of the four subtrees "
                          "around it (rows node1, node2, ... in post-order, after any --unequal-quartets rows; the clades are "
                          "listed in the file's table `clade`).  No depth check either: a lineage through the parent can be "
                          "nearly twice the tree's depth")
    new.add_argument('--exact-quartets', default=False, action='store_true',
                     help="beside the normal approximation of --quartets, --unequal-quartets and --tree-quartets, the exact "
                          "probabilities from the law of the site counts itself (a table `quartet_exact` in each quartet "
                          "database the run writes: p_correct, p_incorrect or p_ac and p_ad, p_polytomy, the window used and "
                          "the bound on the mass outside it; exact to that bound and rounding).  Matters for loci with few "
                          "expected signal sites, where the approximation is off by up to 0.05.  Needs one of those flags")
    new.add_argument('--exact-quartets-window', type=int, default=None, metavar='M',
                     help="largest window of --exact-quartets, a power of two in 16..512 (default 128: variances of the count "
                          "differences up to about 46); a locus and quartet that need a larger one get NULL probabilities "
                          "and window 0, never a truncated answer.  Needs --exact-quartets")
    new.add_argument('--locus-sets', default=False, action='store_true',
                     help="accumulation curves over an ordered list of loci: how likely the first k loci, analysed together, "
                          "are to resolve each quartet, for every k (tables `locus_set` and `locus_set_summary` in each quartet "
                          "database the run writes; with --exact-quartets also `locus_set_exact`, all prefixes on the window "
                          "of --exact-quartets-window).  The default order is per quartet: descending per-locus p_correct of "
                          "the normal approximation, ties by file order.  Needs --quartets, --unequal-quartets or --tree-quartets")
    new.add_argument('--locus-sets-order', action=base.FullPaths, default=None, metavar='FILE',
                     help="one locus name per line (a file's name without its extension): the order of --locus-sets, the same "
                          "for every quartet; loci that are not named are left out.  Needs --locus-sets")
    new.add_argument('--locus-sets-max', type=int, default=None, metavar='K',
                     help="the largest set of --locus-sets: the order is cut to its first K loci (K >= 1; default all).  "
                          "Needs --locus-sets")
    new.add_argument('--locus-sets-target', type=float, default=None, metavar='P',
                     help="the p_correct, in (0, 1), whose smallest sufficient k `locus_set_summary` reports (default 0.95).  "
                          "Needs --locus-sets")
    new.add_argument('--site-concordance', default=False, action='store_true',
                     help="site concordance factors (Minh, Hahn & Lanfear 2020) of every locus at every internode of the input "
                          "tree: what the alignment shows where --tree-quartets predicts.  Per locus and internode the numbers "
                          "of quartets its sites support as ab|cd, ac|bd and ad|bc -- over all quartets of the four groups of "
                          "taxa around the internode (exact, from the groups' base counts), for the nearest-tip quartet of "
                          "--tree-quartets, and sCF, sDF1, sDF2 and sN as means over sampled quartets -- go into "
                          "phylogenetic-informativeness-concordance.sqlite, with the same for all loci together.  Cells that "
                          "are not exactly one base are not decisive.  Not with --site-rates")
    new.add_argument('--site-concordance-quartets', type=int, default=None, metavar='Q',
                     help="sampled quartets per internode, 1..10000 (default 100); an internode with at most Q quartets has all "
                          "of them listed instead.  Needs --site-concordance")
    new.add_argument('--site-concordance-seed', type=int, default=None, metavar='S',
                     help="seed of the sampling (default 1); needs --site-concordance")
    args = parser.parse_args(argv)
    _locus_set_flags(parser, args)
    if args.site_concordance:
        if args.site_rates:
            parser.error("--site-concordance counts the sites of the alignments: it cannot be combined with --site-rates, which reads none")
        if args.site_concordance_quartets is None:
            args.site_concordance_quartets = 100
        if not 1 <= args.site_concordance_quartets <= 10000:
            parser.error("--site-concordance-quartets must be in 1..10000")
        if args.site_concordance_seed is None:
            args.site_concordance_seed = 1
        if not 0 <= args.site_concordance_seed < 2 ** 64:
            parser.error("--site-concordance-seed must be in 0..2^64-1")
    else:
        for flag, value in (('--site-concordance-quartets', args.site_concordance_quartets),
                            ('--site-concordance-seed', args.site_concordance_seed)):
            if value is not None:
                parser.error("{0} needs --site-concordance".format(flag))
    if args.exact_quartets:
        if args.quartets is None and args.unequal_quartets is None and not args.tree_quartets:
            parser.error("--exact-quartets needs --quartets, --unequal-quartets or --tree-quartets")
        if args.exact_quartets_window is None:
            args.exact_quartets_window = 128
        if args.exact_quartets_window not in (16, 32, 64, 128, 256, 512):
            parser.error("--exact-quartets-window must be a power of two in 16..512")
    elif args.exact_quartets_window is not None:
        parser.error("--exact-quartets-window needs --exact-quartets")
    for flag, given in (('--quartets', args.quartets is not None), ('--unequal-quartets', args.unequal_quartets is not None),
                        ('--tree-quartets', args.tree_quartets)):
        if given and args.site_rates and args.site_model == 'locus' and args.exchangeabilities is None:
            parser.error("{0} needs the loci's substitution model, which --site-rates does not read: "
                         "add --site-model jc, --site-model f81 or --exchangeabilities".format(flag))
    if args.bootstrap and not 2 <= args.bootstrap <= 4096:
        parser.error("--bootstrap must be in 2..4096")
    _seed_and_level(parser, args, '--bootstrap')
    if args.parametric_bootstrap:
        if not 2 <= args.parametric_bootstrap <= 4096:
            parser.error("--parametric-bootstrap must be in 2..4096")
        if args.site_rates:
            parser.error("--parametric-bootstrap simulates alignments: it cannot be combined with --site-rates, which reads none")
        if args.rate_estimator == 'eb':
            parser.error("--parametric-bootstrap re-estimates maximum-likelihood rates: it cannot be combined with --rate-estimator eb")
        if args.gamma_categories > 1:
            parser.error("--parametric-bootstrap has no rate mixture: it cannot be combined with --gamma-categories above 1")
    _seed_and_level(parser, args, '--parametric-bootstrap')
    if args.site_model != 'locus':
        for flag, given in (('--exchangeabilities', args.exchangeabilities is not None), ('--subs-model', bool(args.subs_model)),
                            # (with a quartet flag: the model of that stage)
                            ('--site-rates', args.site_rates and args.quartets is None and args.unequal_quartets is None
                             and not args.tree_quartets)):
            if given:
                parser.error("--site-model {0} fixes the model: it cannot be combined with {1}".format(args.site_model, flag))
    eb_flags = (('--eb-categories', args.eb_categories), ('--eb-alpha', args.eb_alpha), ('--eb-alpha-bounds', args.eb_alpha_bounds))
    if args.rate_estimator != 'eb':
        for flag, value in eb_flags:
            if value is not None:
                parser.error("{0} needs --rate-estimator eb".format(flag))
    else:
        if args.site_rates:
            parser.error("--rate-estimator eb estimates the site rates: it cannot be combined with --site-rates")
        if args.gamma_categories > 1:
            parser.error("--rate-estimator eb has its own prior (--eb-categories): it cannot be combined with --gamma-categories above 1")
        if args.eb_categories is None:
            args.eb_categories = 8
        if not 2 <= args.eb_categories <= 16:
            parser.error("--eb-categories must be in 2..16")
        if args.eb_alpha is not None and not args.eb_alpha > 0:
            parser.error("--eb-alpha must be positive")
        if args.eb_alpha_bounds is None:
            args.eb_alpha_bounds = (0.2, 50.0)
        if not 0 < args.eb_alpha_bounds[0] < args.eb_alpha_bounds[1]:
            parser.error("--eb-alpha-bounds must be LO,HI with 0 < LO < HI")
    if args.posterior_pi:
        if args.rate_estimator != 'eb':
            parser.error("--posterior-pi carries the empirical-Bayes rate posterior: it needs --rate-estimator eb")
        if not 2 <= args.posterior_pi <= 4096:
            parser.error("--posterior-pi must be in 2..4096")
    _seed_and_level(parser, args, '--posterior-pi')
    return args


def _locus_set_flags(parser, args):
    """--locus-sets and its three options: given without the stage they are an error, with it they get their defaults and
    their ranges are held."""
    options = (('--locus-sets-order', args.locus_sets_order), ('--locus-sets-max', args.locus_sets_max),
               ('--locus-sets-target', args.locus_sets_target))
    if not args.locus_sets:
        for flag, value in options:
            if value is not None:
                parser.error("{0} needs --locus-sets".format(flag))
        return
    if args.quartets is None and args.unequal_quartets is None and not args.tree_quartets:
        parser.error("--locus-sets needs --quartets, --unequal-quartets or --tree-quartets")
    if args.locus_sets_max is not None and args.locus_sets_max < 1:
        parser.error("--locus-sets-max must be at least 1")
    if args.locus_sets_target is None:
        args.locus_sets_target = 0.95
    if not 0.0 < args.locus_sets_target < 1.0:
        parser.error("--locus-sets-target must be in (0, 1)")


def _seed_and_level(parser, args, flag):
    """The seed and level of a replicate stage (--bootstrap, --parametric-bootstrap, --posterior-pi), after the stage's own
    checks: given without the stage they are an error, with it they get their defaults and their ranges are held."""
    name = flag[2:].replace('-', '_')
    seed, level = getattr(args, name + '_seed'), getattr(args, name + '_level')
    if not getattr(args, name):
        for what, value in (('seed', seed), ('level', level)):
            if value is not None:
                parser.error("{0}-{1} needs {0}".format(flag, what))
        return
    setattr(args, name + '_seed', 1 if seed is None else seed)
    if not 0 <= getattr(args, name + '_seed') < 2 ** 64:
        parser.error("{0}-seed must be in 0..2^64-1".format(flag))
    setattr(args, name + '_level', 0.95 if level is None else level)
    if not 0.0 < getattr(args, name + '_level') < 1.0:
        parser.error("{0}-level must be in (0, 1)".format(flag))


def _six_floats(string):
    try:
        v = [float(x) for x in string.split(',')]
        assert len(v) == 6
    except Exception as e:
        raise argparse.ArgumentTypeError("Cannot convert exchangeabilities to six numbers: {0}".format(e))
    return v


def _quartets(string):
    """T:to[,T:to...] -> [(label as typed, T, to)]"""
    out = []
    for item in string.split(','):
        try:
            a, b = item.split(':')
            tip, internode = float(a), float(b)
        except Exception:
            raise argparse.ArgumentTypeError("Cannot convert quartet %r to T:to (two numbers)" % item)
        if not (np.isfinite(tip) and np.isfinite(internode)):
            raise argparse.ArgumentTypeError("quartet %r: T and to must be finite" % item)
        if not internode > 0:
            raise argparse.ArgumentTypeError("quartet %r: the internode length to must be positive" % item)
        if not tip >= 0:
            raise argparse.ArgumentTypeError("quartet %r: the tip length T must not be negative" % item)
        out.append((item.strip(), tip, internode))
    if not 1 <= len(out) <= 256:
        raise argparse.ArgumentTypeError("--quartets takes 1..256 quartets")
    return out


def _unequal_quartets(string):
    """Ta/Tb/Tc/Td:to[,...] -> [(label as typed, Ta, Tb, Tc, Td, to)]"""
    out = []
    for item in string.split(','):
        try:
            tips, b = item.split(':')
            ta, tb, tc, td = (float(v) for v in tips.split('/'))
            internode = float(b)
        except Exception:
            raise argparse.ArgumentTypeError("Cannot convert quartet %r to Ta/Tb/Tc/Td:to (five numbers)" % item)
        if not np.all(np.isfinite([ta, tb, tc, td, internode])):
            raise argparse.ArgumentTypeError("quartet %r: Ta, Tb, Tc, Td and to must be finite" % item)
        if not internode > 0:
            raise argparse.ArgumentTypeError("quartet %r: the internode length to must be positive" % item)
        for name, tip in zip(("Ta", "Tb", "Tc", "Td"), (ta, tb, tc, td)):
            if not tip >= 0:
                raise argparse.ArgumentTypeError("quartet %r: the tip length %s must not be negative" % (item, name))
        out.append((item.strip(), ta, tb, tc, td, internode))
    if not 1 <= len(out) <= 256:
        raise argparse.ArgumentTypeError("--unequal-quartets takes 1..256 quartets")
    return out


def _two_floats(string):
    try:
        v = tuple(float(x) for x in string.split(','))
        assert len(v) == 2
    except Exception as e:
        raise argparse.ArgumentTypeError("Cannot convert bounds to two numbers: {0}".format(e))
    return v


def welcome_message():
    return '''
    ***************************************************
    *                                                 *
    * tapir: high-throughput estimates of             *
    * phylogenetic informativeness                    *
    *                                                 *
    * MI355X engine (tapir_amd): site-rate ML and PI  *
    * in one HIP pipeline.  Method credits:           *
    *                                                 *
    *   - J.P. Townsend, 2007. Profiling              *
    *     phylogenetic informativeness. Systematic    *
    *     Biology, 56(2), 222-231.                    *
    *                                                 *
    *   - Pond, S.L.K., Frost, S.D.W., and S.V. Muse, *
    *     2005. Hyphy: hypothesis testing using       *
    *     phylogenies. Bioinformatics, 21(5), 676-9.  *
    *                                                 *
    *   - B.C. Faircloth, J. Chang, M.E. Alfaro, 2012.*
    *     TAPIR (the program this engine drops into). *
    *                                                 *
    ***************************************************\n\n'''


def read_subs_model(path, alignments):
    table = {}
    with open(path) as fh:
        for line in fh:
            parts = line.rstrip("\n").split("\t")
            if len(parts) >= 7 and not line.startswith("#"):
                table[parts[0]] = [float(x) for x in parts[1:]]
    exch, pi = [], []
    for a in alignments:
        b = os.path.basename(a)
        if b not in table:
            raise IOError("no substitution model for {0} in {1}".format(b, path))
        exch.append(table[b][:6])
        pi.append(table[b][6:10] if len(table[b]) >= 10 else None)
    pis = None if any(p is None for p in pi) else np.array(pi)
    return np.array(exch), pis


def _broadcast(obj, rank, world):
    if world == 1:
        return obj
    import torch.distributed as dist
    box = [obj if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return box[0]


def _gather_rows(tables, nfiles, rank, world, on_gpu):
    """[n_local, W] rows of this rank's files (file i -> rank i mod world) -> [nfiles, W] in file order."""
    if world == 1:
        return tables
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tables, dtype=np.float64))
    if on_gpu:
        t = t.cuda()
    return tdist.gather_tables(t, nfiles, rank, world).cpu().numpy()


def main(argv=None, engine_mod=None):
    """Main loop (mirrors bin/tapir_compute.py:125-177)."""
    args = get_args(argv)
    rank, world = tdist.rank_world()
    on_gpu = engine_mod is None
    pool = None
    if args.multiprocessing:  # the reference: Pool(processes = cpu_count() - 1), bin/tapir_compute.py:162-163
        from multiprocessing import cpu_count
        # forked here, before torch.distributed / RCCL and before the first libtphip call: see pipeline.HostPool
        # (forking hundreds of workers costs more than it saves: at most 16 per rank)
        pool = pipeline.HostPool(max(1, min(16, (cpu_count() - 1) // world)))
    try:
        return _main(args, rank, world, on_gpu, engine_mod, pool)
    finally:
        if pool is not None:
            pool.close()


class _ProbeDb:
    """phylogenetic-informativeness.sqlite: opened at the first call, committed and closed by close(), its seconds in
    LAST_TIMINGS["sqlite"].  Whole on one thread (sqlite objects live and die on the thread that made them): the main one,
    or the one run_alignments hands store() or add() / close() to while the `.rates` files are written."""

    def __init__(self, name, run):
        self.name, self.run, self.conn, self.seconds = name, run, None, 0.0

    def _timed(self, fn, *rows):
        import time
        t0 = time.perf_counter()
        if self.conn is None:
            self.conn, self.c = db.create_probe_db(self.name)
        fn(self.conn, self.c, *rows)
        self.seconds += time.perf_counter() - t0

    def add(self, names, tables):   # rows block by block, in file order (pipeline._run_streamed), or all at once
        self._timed(db.insert_tables, names, tables, self.run.T, self.run.times, self.run.intervals)

    def store(self, pis):   # tapir_compute.py's last step
        self._timed(db.insert_pi_data, pis)
        self.close()

    def close(self):
        self._timed(lambda conn, c: (conn.commit(), c.close(), conn.close()))
        LAST_TIMINGS["sqlite"] = self.seconds


@dataclasses.dataclass
class _Stage:
    """What the opt-in stages after the main database work on, in one process: every rank takes its own loci (`mine`, the
    global file indices `ids`: the generators' stream ids, so nothing depends on the world size) with their final rates and
    the models and fits of its own run; rank 0 writes the stage's database."""
    args: object
    rank: int
    world: int
    on_gpu: bool
    eng: object
    run: pipeline.Run
    files: list
    mine: list
    ids: list
    per_locus: list
    models: dict
    ebfit: dict
    subsets: dict

    def gather(self, rows):
        """[n_local, ...] rows of this rank's files -> [nfiles, ...] in file order: the one collective of a stage (none when
        a row is empty: a tree without an internode and nothing typed)."""
        shape, n = rows.shape[1:], len(self.files)
        width = int(np.prod(shape))
        if width == 0:
            return np.zeros((n,) + shape)
        return _gather_rows(rows.reshape(len(self.ids), width), n, self.rank, self.world, self.on_gpu).reshape((n,) + shape)

    def stage_models(self):
        """The loci's models: the main run's (a rank without loci: none); under --site-rates, which reads rates only,
        Jukes-Cantor, or the base frequencies the `.rates` documents carry with exchangeabilities of 1 (f81) or the
        --exchangeabilities given."""
        args, L = self.args, len(self.mine)
        if not args.site_rates:
            return self.models if self.models is not None else dict(
                pi=np.zeros((0, 4)), exch=np.zeros((0, 6)), model="gtr" if args.site_model == 'locus' else "f81")
        if args.site_model == 'jc':
            return dict(pi=np.full((L, 4), 0.25), exch=None, model="f81")
        import json
        pi = np.empty((L, 4))
        for l, f in enumerate(self.mine):
            with open(f) as fh:
                freqs = json.load(fh)["sites"].get("freqs")
            if not freqs:
                raise IOError("{0} carries no base frequencies (\"freqs\"): --quartets can only use --site-model jc with it".format(f))
            pi[l] = [freqs[k] for k in "ACGT"]
        if args.site_model == 'f81':
            return dict(pi=pi, exch=None, model="f81")
        return dict(pi=pi, exch=np.tile(np.array(args.exchangeabilities, dtype=np.float64), (L, 1)), model="gtr")

    def path(self, name):
        return os.path.join(self.args.output, name)


def _main(args, rank, world, on_gpu, engine_mod, pool):
    if world > 1:
        tdist.init_process_group(None if on_gpu else "gloo")
        if on_gpu:
            args.device = int(os.environ.get("LOCAL_RANK", rank))
    if rank == 0:
        print(welcome_message())
        args.output = base.create_unique_dir(args.output)
        # correct branch lengths
        setup = (args.output,) + tuple(compute.correct_branch_lengths(args.tree, args.tree_format, d=args.output))
    else:
        setup = None
    args.output, tree_depth, correction, tree = _broadcast(setup, rank, world)
    for label, tip, internode in args.quartets or []:
        if tip + internode > tree_depth:
            raise ValueError("--quartets {0}: T + to = {1} exceeds the tree depth {2}".format(label, tip + internode, tree_depth))
    subset_pi = dict()
    if args.subset_pi_map_file:
        subset_pi = dict(base.parse_subset_map_file(args.subset_pi_map_file))
    root = newick.read_tree(tree, 'newick')
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    cat_rates, cat_weights = (compute.discrete_gamma(args.gamma_alpha, args.gamma_categories)
                              if args.gamma_categories > 1 else (None, None))
    # T: a vector of times given start and stops
    run = pipeline.Run(leaf_names, parent, blen, leaf, int(tree_depth), args.times, args.intervals, correction=correction,
                       threshold=args.threshold, round_decimals=-1 if args.full_precision_rates else 4,
                       integ_mode=0 if args.integral_mode == 'quadpack' else 1, device=args.device,
                       start_rule=1 if args.reference_start else 0, cat_rates=cat_rates, cat_weights=cat_weights)
    eng = engine_mod
    if eng is None:
        from . import engine as eng
    progress = pipeline.dot_progress if rank == 0 else None
    db_name = os.path.join(args.output, 'phylogenetic-informativeness.sqlite')
    probe_db = _ProbeDb(db_name, run)
    stored = False
    pis, tables, models, ebfit = [], np.zeros((0, run.width)), None, None
    if rank == 0:
        print("Estimating PI for files (--site-rate option):" if args.site_rates else "\nEstimating site rates and PI for files:")
    files = base.get_files(args.alignments, '*.rates' if args.site_rates else '*.nex,*.nexus')
    ids = list(tdist.shard_loci(len(files), rank, world))
    mine = [files[i] for i in ids]
    if mine and args.site_rates:
        pis, tables = pipeline.run_rate_files(mine, run, subsets=subset_pi, engine_mod=eng, progress=progress, return_tables=True)
    elif mine:
        exch, pi = None, None  # None: fit and model-average the exchangeabilities per locus (HyPhy stage 1)
        if args.exchangeabilities is not None:
            exch = np.array(args.exchangeabilities)
        if args.subs_model:
            exch, pi = read_subs_model(args.subs_model, mine)
        # single process: the database may be written while the pool writes the .rates files
        pis, out = pipeline.run_alignments(mine, run, exch, pi=pi, subsets=subset_pi, output_dir=args.output, engine_mod=eng,
                                           progress=progress, pool=pool,
                                           during_write=probe_db.store if world == 1 else None,
                                           table_sink=probe_db if world == 1 else None,
                                           site_model=args.site_model, rate_estimator=args.rate_estimator,
                                           eb_options=None if args.rate_estimator != 'eb' else dict(
                                               categories=args.eb_categories, alpha=args.eb_alpha,
                                               alpha_bounds=args.eb_alpha_bounds))
        tables = out["final_tables"]
        models = out.get("models")
        ebfit = out.get("eb")
        stored = bool(out.get("during_write_done"))
        sqlite_seconds = LAST_TIMINGS.get("sqlite")
        LAST_TIMINGS.clear()
        LAST_TIMINGS.update(out.get("timings", {}))
        if stored:
            LAST_TIMINGS["sqlite"] = sqlite_seconds
    cx = _Stage(args, rank, world, on_gpu, eng, run, files, mine, ids, [p[1] for p in pis], models, ebfit, subset_pi)
    # the one collective of the main run: every rank's PI rows -> all rows in file order
    all_tables = cx.gather(tables)
    if rank == 0:
        # store results somewhere
        sys.stdout.write("\nStoring results in {0}...".format(db_name))
        sys.stdout.flush()
        if world > 1:
            probe_db.add(files, all_tables)
            probe_db.close()
        elif not stored:
            probe_db.store(pis)
        sys.stdout.write("DONE")
        sys.stdout.flush()
        print("\n")
    # (after the main database is stored: a failure of an opt-in stage leaves a finished run's outputs in place)
    if args.bootstrap:
        _bootstrap_stage(cx)
    if args.parametric_bootstrap:
        _parametric_bootstrap_stage(cx)
    if args.posterior_pi:
        _posterior_pi_stage(cx)
    if args.quartets:
        _quartets_stage(cx)
    if args.unequal_quartets or args.tree_quartets:
        _unequal_quartets_stage(cx)
    if args.site_concordance:
        _concordance_stage(cx)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return args.output


def _bootstrap_stage(cx):
    """--bootstrap: every rank resamples its own loci from their final rates; the summaries travel like the PI rows."""
    args, run = cx.args, cx.run
    boot = pipeline.bootstrap_tables(cx.eng, cx.per_locus, run, cx.ids, args.bootstrap, args.bootstrap_seed, args.bootstrap_level)
    all_boot = cx.gather(boot)
    if cx.rank == 0:
        db.write_bootstrap_db(cx.path('phylogenetic-informativeness-bootstrap.sqlite'), cx.files, all_boot, run.T, run.times,
                              run.intervals, args.bootstrap, args.bootstrap_seed, args.bootstrap_level)


def _parametric_bootstrap_stage(cx):
    """--parametric-bootstrap: as the site bootstrap; the alignments are re-read: the main run does not keep them."""
    args, run = cx.args, cx.run
    pboot, _ = pipeline.parametric_bootstrap_tables(
        cx.eng, cx.mine, cx.per_locus, cx.stage_models(), run, cx.ids, args.parametric_bootstrap, args.parametric_bootstrap_seed,
        args.parametric_bootstrap_level, subsets=cx.subsets, output_dir=args.output)
    all_pboot = cx.gather(pboot)
    if cx.rank == 0:
        db.write_bootstrap_db(cx.path('phylogenetic-informativeness-parametric-bootstrap.sqlite'), cx.files, all_pboot, run.T,
                              run.times, run.intervals, args.parametric_bootstrap, args.parametric_bootstrap_seed,
                              args.parametric_bootstrap_level, method="parametric")


def _posterior_pi_stage(cx):
    """--posterior-pi: as the parametric bootstrap, with the fits of the rank's own run; bands, categories and fits travel as
    one row per locus."""
    args, run, n = cx.args, cx.run, len(cx.ids)
    Wb, K = run.band_width, args.eb_categories
    fit = cx.ebfit if cx.ebfit is not None else dict(alpha=np.zeros(0), scale=np.zeros(0), categories=K)
    post = pipeline.posterior_pi_tables(cx.eng, cx.mine, cx.per_locus, cx.stage_models(), fit, run, cx.ids, args.posterior_pi,
                                        args.posterior_pi_seed, args.posterior_pi_level, subsets=cx.subsets)
    packed = np.concatenate([post["bands"].reshape(n, 4 * Wb), post["category_rate"].reshape(n, K),
                             post["expected_sites"].reshape(n, K), np.asarray(fit["alpha"], dtype=np.float64).reshape(n, 1),
                             np.asarray(fit["scale"], dtype=np.float64).reshape(n, 1)], axis=1)
    all_post = cx.gather(packed)
    if cx.rank == 0:
        bands, cat_rate, sites, alpha, scale = np.split(all_post, [4 * Wb, 4 * Wb + K, 4 * Wb + 2 * K, 4 * Wb + 2 * K + 1], axis=1)
        db.write_posterior_db(cx.path('phylogenetic-informativeness-posterior.sqlite'), cx.files,
                              bands.reshape(len(cx.files), 4, Wb), cat_rate, sites, alpha[:, 0], scale[:, 0], run.T, run.times,
                              run.intervals, args.posterior_pi, args.posterior_pi_seed, args.posterior_pi_level)


def _quartets_stage(cx):
    """--quartets (and their exact probabilities): from every rank's final rates; rows travel like the PI rows."""
    args, models = cx.args, cx.stage_models()
    labels = [q[0] for q in args.quartets]
    lengths = np.array([[q[1], q[2]] for q in args.quartets], dtype=np.float64)
    call = (cx.eng, cx.per_locus, models["pi"], models["exch"], cx.run, lengths)
    all_rows = cx.gather(pipeline.quartet_tables(*call, model=models["model"]))
    if args.exact_quartets:
        all_exact = cx.gather(pipeline.exact_quartet_tables(*call, model=models["model"], window_cap=args.exact_quartets_window))
    if cx.rank == 0:
        name = cx.path('phylogenetic-informativeness-quartets.sqlite')
        db.write_quartet_db(name, cx.files, all_rows, labels, lengths, models["model"])
        if args.exact_quartets:
            db.add_quartet_exact_table(name, all_exact, labels, args.exact_quartets_window)
    if args.locus_sets:
        _locus_sets(cx, cx.path('phylogenetic-informativeness-quartets.sqlite'), all_rows, labels, lengths, models, False)


def _unequal_quartets_stage(cx):
    """--unequal-quartets / --tree-quartets: as --quartets; the typed rows first, then the input tree's internodes, read in
    the tree's original units."""
    args, models = cx.args, cx.stage_models()
    typed = args.unequal_quartets or []
    of_tree = compute.tree_quartets(newick.read_tree(args.tree, args.tree_format)) if args.tree_quartets else []
    labels = [q[0] for q in typed] + [q[0] for q in of_tree]
    lengths = np.array([q[1:6] for q in typed] + [q[2:7] for q in of_tree], dtype=np.float64).reshape(-1, 5)
    call = (cx.eng, cx.per_locus, models["pi"], models["exch"], cx.run, lengths)
    all_rows = cx.gather(pipeline.unequal_quartet_tables(*call, model=models["model"]))
    if args.exact_quartets:
        all_exact = cx.gather(pipeline.exact_unequal_quartet_tables(*call, model=models["model"],
                                                                    window_cap=args.exact_quartets_window))
    if cx.rank == 0:
        name = cx.path('phylogenetic-informativeness-unequal-quartets.sqlite')
        db.write_unequal_quartet_db(name, cx.files, all_rows, labels, lengths, models["model"],
                                    clades=[(q[0], q[1]) for q in of_tree])
        if args.exact_quartets:
            db.add_quartet_exact_table(name, all_exact, labels, args.exact_quartets_window, unequal=True)
    if args.locus_sets:
        _locus_sets(cx, cx.path('phylogenetic-informativeness-unequal-quartets.sqlite'), all_rows, labels, lengths, models, True)


def _gather_objects(obj, rank, world):
    """Every rank's picklable object -> the list of them on rank 0 (None elsewhere)."""
    if world == 1:
        return [obj]
    import torch.distributed as dist
    box = [None] * world if rank == 0 else None
    dist.gather_object(obj, box, dst=0)
    return box


def _concordance_stage(cx):
    """--site-concordance: every rank counts its own loci over sets that are the same everywhere; the rows travel like the PI
    rows, the ranks' integer totals as objects to rank 0, which adds them and forms the rows of all loci together.  The input
    tree is read as it is, like --tree-quartets; a tree without an internode gives empty tables and no engine call."""
    args = cx.args
    root = newick.read_tree(args.tree, args.tree_format)
    groups = compute.tree_concordance_groups(root)
    sets = compute.concordance_sets(groups, cx.run.leaf_names, args.site_concordance_quartets, args.site_concordance_seed)
    rows, totals = pipeline.concordance_tables(cx.eng, cx.mine, cx.per_locus, cx.run, sets, subsets=cx.subsets)
    all_rows = cx.gather(rows)
    parts = _gather_objects(totals, cx.rank, cx.world)
    if cx.rank != 0:
        return
    both = np.zeros((len(groups), 12))
    if len(groups) and len(cx.files):
        total = [[sum(int(p[s, k]) for p in parts) for k in range(3)] for s in range(len(totals))]
        if max(max(t) for t in total) >= 2 ** 53:
            raise pipeline.PipelineError("the concordance counts of all loci together reach 2^53: they would not convert exactly")
        both = cx.eng.concordance_rows(np.array(total, dtype=np.uint64).reshape(1, len(total), 3), sets["node_sets"],
                                       device=cx.run.device)[0]
    db.write_concordance_db(cx.path('phylogenetic-informativeness-concordance.sqlite'), cx.files, all_rows, both, groups, sets,
                            args.site_concordance_quartets, args.site_concordance_seed,
                            clades=[(q[0], q[1]) for q in compute.tree_quartets(root)])


def _locus_sets(cx, name, all_rows, labels, lengths, models, unequal):
    """--locus-sets, after a quartet stage has written `name`: the order from the gathered per-locus rows (every rank has them and
    finds the same order), the normal rows on rank 0, and with --exact-quartets the exact rows on rank 0 too, from the final
    rates and models of the loci the orders name, which travel there from the ranks that own them -- the sub-batch is the
    same whatever the world size, so the rows are the same bits."""
    args = cx.args
    if len(cx.files) == 0 or len(labels) == 0:
        return
    order = pipeline.locus_set_order(all_rows, [db.locus_name(f) for f in cx.files], args.locus_sets_order, args.locus_sets_max)
    exact = None
    if args.exact_quartets:
        union = np.unique(order)
        wanted = set(union.tolist())
        pi, exch = models["pi"], models["exch"]
        mine = {int(g): (cx.per_locus[l], np.asarray(pi[l], dtype=np.float64), None if exch is None else np.asarray(exch[l], dtype=np.float64))
                for l, g in enumerate(cx.ids) if int(g) in wanted}
        parts = _gather_objects(mine, cx.rank, cx.world)
        if cx.rank == 0:
            have = {g: v for part in parts for g, v in part.items()}
            chosen = [have[int(g)] for g in union]
            exact = pipeline.exact_locus_set_tables(
                cx.eng, [v[0] for v in chosen], np.array([v[1] for v in chosen]),
                None if models["model"] != "gtr" else np.array([v[2] for v in chosen]), cx.run, lengths,
                np.searchsorted(union, order), model=models["model"], window_cap=args.exact_quartets_window, unequal=unequal)
    if cx.rank == 0:
        rows = pipeline.locus_set_tables(cx.eng, all_rows, order, cx.run.device)
        db.add_locus_set_tables(name, rows, order, labels, args.locus_sets_target,
                                "p_correct" if args.locus_sets_order is None else "file:" + os.path.basename(args.locus_sets_order),
                                args.locus_sets_max, unequal=unequal, exact=exact,
                                window_cap=args.exact_quartets_window if args.exact_quartets else None)


if __name__ == '__main__':
    main()
