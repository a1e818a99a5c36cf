"""Writes tests/golden/geometry_departures.json: where the compiled reference, as it stands, departs from the same reference with uncached distance
queries in its generator and in its error correction's distance check (oracle/Makefile: _ref/libmsdfgen_ref_exact.so), on the outline families of tests/geomcases.py. Per case and setting:
the values and stencil texels that differ, with both sides' bits; settings of a case with equal lists share one entry. tests/test_geom_cases.py asserts this list, so a change of either build shows.

    python tools/make_golden_geometry.py            # needs both builds under oracle/_ref
    python tools/make_golden_geometry.py --premises # prints what check_premise() counts, for geomcases.MIN_COUNT
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geomcases as G                                          # noqa: E402
from oracle.pyoracle import Oracle, Ref                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "geometry_departures.json")


def main():
    if "--premises" in sys.argv:
        orc = Oracle()
        for c in G.cases():
            print('"%s": %d,' % (c.name, G.premise_count(c, orc)))
        return
    literal, exact = Ref(), Ref(exact=True)
    doc = {"reference": literal.version(), "cases": {}}
    texels = settings = 0
    for c in G.reference_cases():
        d = G.departures(literal, exact, c)
        if d:
            entries, index = [], {}
            for key, v in d.items():
                blob = json.dumps(v, sort_keys=True)
                if blob not in index:
                    index[blob] = len(entries)
                    entries.append(v)
            doc["cases"][c.name] = {"entries": entries, "settings": {key: index[json.dumps(v, sort_keys=True)] for key, v in d.items()}}
            settings += len(d)
            texels += sum(len(v["at"]) for v in d.values())
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d settings, %d values, %d bytes" % (OUT, len(doc["cases"]), settings, texels, os.path.getsize(OUT)))
    for name, d in doc["cases"].items():
        print("  %-44s %3d settings, %d distinct, at most %d values, check modes %s" % (name, len(d["settings"]), len(d["entries"]),
              max(len(v["at"]) for v in d["entries"]), sorted({k.split("/")[-1] for k in d["settings"]})))


if __name__ == "__main__":
    main()
