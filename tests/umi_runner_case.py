"""TEST INFRASTRUCTURE: the end-to-end case of the UMI tests -- a dozen hand-made reads for a kit whose start adapter carries a
sixteen-base UMI in four blocks and whose end adapter an eight-base one -- with the output FASTQ and the UMI report STATED
BY HAND from where the instances were planted (extra_end_trim 2; a start adapter in the middle takes 100 bases before it and 10
behind it).  The CPU test runs it on tests/umi_aligner.py, the GPU test on the library; both must write these bytes."""
import random

PREFIX, SUFFIX = "CAAGCAGAAGACGGCATACGAGAT", "GTGACTGGAGTTCAG"
START = PREFIX + "TTTVVVVTTVVVVTTVVVVTTVVVVTTT" + SUFFIX       # 67 rows; rows 27 .. 48 are the span: four blocks of V = ACG with TT between
END = "GCTAGTCAGGTC" + "NNNNNNNN" + "CTGATCCATGAGTC"   # rows 12 .. 19
KIT = "UMI kit"
BODY = 240
CHIMERA_BODY = 1500


def adapter_sets():
    from porechop_amd.pipeline import AdapterSet
    return [AdapterSet(KIT, ("UMI_start", START), ("UMI_end", END))]


def start_instance(u):
    """The start adapter with the sixteen bases u (A/C/G) under its V rows."""
    assert len(u) == 16 and set(u) <= set("ACG")
    return PREFIX + "TTT" + u[0:4] + "TT" + u[4:8] + "TT" + u[8:12] + "TT" + u[12:16] + "TTT" + SUFFIX


def start_umi(u):
    """What lies under rows 27 .. 48 of that instance: the blocks with the fixed TT rows between them."""
    return u[0:4] + "TT" + u[4:8] + "TT" + u[8:12] + "TT" + u[12:16]


def end_instance(u):
    assert len(u) == 8
    return "GCTAGTCAGGTC" + u + "CTGATCCATGAGTC"


def _body(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def build():
    """-> (records [(header, sequence)], expected output records [(header, sequence)], expected report rows [tuple])"""
    rng = random.Random(1616)
    reads, out, rows = [], [], []

    def add(header, start_u, end_u, body, clipped=0, insert=None):
        name = header.split(" ")[0]
        head = ""
        tags = []
        if start_u is not None:
            head = start_instance(start_u)
            umi = start_umi(start_u)
            if insert is not None:                   # a base inserted inside the span: one column more under it
                head = head[:insert] + "A" + head[insert:]
                umi = head[27:50]
            head = head[clipped:]
            if not clipped:
                tags.append("UMI_start=" + umi)
                rows.append((name, "start", KIT, 27, len(umi), 22, 22, umi))
        tail = end_instance(end_u) if end_u is not None else ""
        seq = head + body + tail
        if end_u is not None:
            tags.append("UMI_end=" + end_u)
            rows.append((name, "end", KIT, len(seq) - len(END) + 12, 8, 8, 8, end_u))
        reads.append((header, seq))
        return seq, tags

    def plain(header, start_u, end_u, **kw):
        body = _body(rng, BODY)
        seq, tags = add(header, start_u, end_u, body, **kw)
        kept = body[2 if start_u is not None else 0:len(body) - (2 if end_u is not None else 0)]     # adapter + extra_end_trim
        out.append((" ".join([header] + tags), kept))

    plain("read_1", "ACGACGACGACGACGA", "ACGTACGT")                 # both ends
    plain("read_2", "GGGGCCCCAAAAGCGC", "TTTTGGGG")
    plain("read_3", "CACACACAGAGAGAGA", "NACGTTGA", insert=35)       # an inserted base in the start UMI; an N in the end UMI stays an N
    plain("read_4", "AAAACCCCGGGGACGA", None)                       # the start only
    plain("read_5", "CGCGCGCGACACAGAG", None)
    plain("read_6", None, "GATTACAG")                               # the end only
    plain("read_7", None, "CCCCCCCC")
    plain("read_8", None, None)                                     # neither
    plain("read_9", None, None)
    plain("read_10", "ACGACGACGACGACGA", None, clipped=36)          # the read starts inside the instance: trimmed, no UMI
    plain("read_11 runid=7 ch=12", "GACGACGACGACGACG", "ACACACAC")  # a header with a comment: the tags go behind it
    # a chimera: the start adapter once more in its middle -- two pieces, both with the read's tags
    b1, b2 = _body(rng, CHIMERA_BODY), _body(rng, CHIMERA_BODY)
    _, tags = add("read_12 ch=5", "AGAGAGAGCACACACA", "GTGTGTGT", b1 + start_instance("ACGACGACGACGACGA") + b2)
    out.append((" ".join(["read_12_1 ch=5"] + tags), b1[2:len(b1) - 100]))
    out.append((" ".join(["read_12_2 ch=5"] + tags), b2[10:-2]))
    return reads, out, rows


def fastq_text(records):
    return "".join("@%s\n%s\n+\n%s\n" % (h, s, "5" * len(s)) for h, s in records)


def report_text(rows):
    return "#name\tside\tset\tread_first\tlength\tcovered\tspan_length\tumi\n" + "".join("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % r for r in rows)
