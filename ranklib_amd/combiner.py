"""ciir.umass.edu.learning.Combiner (learning/Combiner.java:21-46): merges the Random Forests models of a directory -- bags trained in
separate runs -- into one model file: "## Random Forests", then the first ensemble of every file.

    python -m ranklib_amd.combiner <directory> <output file>

Files whose name contains ".progress" are skipped, as written.  Three deviations, stated in DESIGN.md 22: the names are sorted (the Java
takes File.list()'s unspecified order); a file that is not a Random Forests model is a RankLibError that names it (the Java ends in a
ClassCastException, or in whatever its loader throws); and a file is read with RFRanker.ensembleBlocks -- the part of
RFRanker.loadFromString that cuts the text into bags -- without building the scoring model on a device, so bags merge on a machine that has
none.  The merged file is checked when it is loaded.
"""
import logging
import os
import sys

from ._native import RankLibError
from .learning import RankerFactory, RFRanker

logger = logging.getLogger("ranklib_amd")


class Combiner:
    def combine(self, directory, outputFile):                        # :28-45
        rf = RankerFactory()
        try:
            fns = sorted(os.listdir(directory))
        except OSError as ex:
            raise RankLibError("Error in Combiner::combine(): %s" % ex)
        out = ["## " + RFRanker().name() + "\n"]
        for fn2 in fns:
            if fn2.find(".progress") != -1:
                continue
            fn = os.path.join(directory, fn2)
            try:
                with open(fn, "r", encoding="ascii") as f:
                    text = f.read()
                first = text.split("\n", 1)[0]
                if rf.names.get(first.replace("## ", "").strip().upper()) != "RANDOM_FOREST":      # RankerFactory.loadRankerFromString :108-118
                    raise RankLibError("its first line is %r, not '## Random Forests'" % first)
                out.append(RFRanker.ensembleBlocks(text)[0] + "\n")                                 # r.getEnsembles()[0].toString()
            except (OSError, UnicodeDecodeError, RankLibError) as ex:
                raise RankLibError("Error in Combiner::combine(): %s is not a Random Forests model: %s" % (fn, ex))
        with open(outputFile, "w", encoding="ascii") as f:
            f.write("".join(out))


def main(argv=None):                  # :23-26
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if len(args) != 2:
        print("Usage: python -m ranklib_amd.combiner <directory of Random Forests models> <output file>")
        return 0
    Combiner().combine(args[0], args[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
