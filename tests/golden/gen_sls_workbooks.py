"""Writes tests/golden/sls_excel/{Processed_Circle_test,Process_parameters}.xlsx: stand-ins for the
reference's two workbooks (models/CvT(Par).py:60-64) in the layout pandas' to_excel gives them
(an unnamed index column, header names as shared strings, numbers as plain <v> cells, a missing
measurement as an absent cell), with drawn values: 200 pieces x every frequency column, 40
process-parameter rows.  Standard library only; the output is byte-stable (fixed zip dates).

    python tests/golden/gen_sls_workbooks.py
"""
import os
import sys
import zipfile
from xml.sax.saxutils import escape

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "transformer-stm_amd"))
from vitmi.sls import FREQUENCIES, PROCESS_PARAMETERS  # noqa: E402

NS = "http://schemas.openxmlformats.org/spreadsheetml/2006/main"
CONTENT_TYPES = ('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>'
                 '<Types xmlns="http://schemas.openxmlformats.org/package/2006/content-types">'
                 '<Default Extension="rels" ContentType="application/vnd.openxmlformats-package.relationships+xml"/>'
                 '<Default Extension="xml" ContentType="application/xml"/>'
                 '<Override PartName="/xl/workbook.xml" ContentType="application/vnd.openxmlformats-officedocument.'
                 'spreadsheetml.sheet.main+xml"/>'
                 '<Override PartName="/xl/worksheets/sheet1.xml" ContentType="application/vnd.openxmlformats-'
                 'officedocument.spreadsheetml.worksheet+xml"/>'
                 '<Override PartName="/xl/sharedStrings.xml" ContentType="application/vnd.openxmlformats-'
                 'officedocument.spreadsheetml.sharedStrings+xml"/></Types>')
RELS = ('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>'
        '<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">'
        '<Relationship Id="rId1" Type="http://schemas.openxmlformats.org/officeDocument/2006/relationships/'
        'officeDocument" Target="xl/workbook.xml"/></Relationships>')
WORKBOOK = ('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>'
            f'<workbook xmlns="{NS}" xmlns:r="http://schemas.openxmlformats.org/officeDocument/2006/relationships">'
            '<sheets><sheet name="Sheet1" sheetId="1" r:id="rId1"/></sheets></workbook>')
WORKBOOK_RELS = ('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>'
                 '<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">'
                 '<Relationship Id="rId1" Type="http://schemas.openxmlformats.org/officeDocument/2006/relationships/'
                 'worksheet" Target="worksheets/sheet1.xml"/>'
                 '<Relationship Id="rId2" Type="http://schemas.openxmlformats.org/officeDocument/2006/relationships/'
                 'sharedStrings" Target="sharedStrings.xml"/></Relationships>')


def col_letters(i):
    s = ""
    i += 1
    while i:
        i, r = divmod(i - 1, 26)
        s = chr(65 + r) + s
    return s


def write_xlsx(path, header, table):
    """header: names of columns 1..; column 0 is the unnamed index 0..n-1.  NaN -> no cell."""
    rows = ['<row r="1">' + "".join(f'<c r="{col_letters(j + 1)}1" t="s"><v>{j}</v></c>' for j in range(len(header)))
            + "</row>"]
    for i, vals in enumerate(table):
        cells = [f'<c r="A{i + 2}"><v>{i}</v></c>']
        cells += [f'<c r="{col_letters(j + 1)}{i + 2}"><v>{v!r}</v></c>' for j, v in enumerate(vals) if v == v]
        rows.append(f'<row r="{i + 2}">' + "".join(cells) + "</row>")
    sheet = (f'<?xml version="1.0" encoding="UTF-8" standalone="yes"?><worksheet xmlns="{NS}"><sheetData>'
             + "".join(rows) + "</sheetData></worksheet>")
    shared = (f'<?xml version="1.0" encoding="UTF-8" standalone="yes"?><sst xmlns="{NS}" count="{len(header)}" '
              f'uniqueCount="{len(header)}">' + "".join(f"<si><t>{escape(h)}</t></si>" for h in header) + "</sst>")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, text in (("[Content_Types].xml", CONTENT_TYPES), ("_rels/.rels", RELS), ("xl/workbook.xml", WORKBOOK),
                           ("xl/_rels/workbook.xml.rels", WORKBOOK_RELS), ("xl/sharedStrings.xml", shared),
                           ("xl/worksheets/sheet1.xml", sheet)):
            info = zipfile.ZipInfo(name, date_time=(2020, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, text.encode("utf-8"))


def main():
    out = os.path.join(HERE, "sls_excel")
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(20)
    pieces, groups = 200, 40
    lab = np.round(rng.normal(1000, 50, (pieces, len(FREQUENCIES))), 3)
    lab[rng.random(lab.shape) < 0.15] = np.nan            # measurements that failed
    lab[35:40] = np.nan                                   # one group of five with no valid piece at all
    write_xlsx(os.path.join(out, "Processed_Circle_test.xlsx"), FREQUENCIES, lab.tolist())
    proc = np.stack([rng.choice([1000.0, 500.0], groups), rng.choice([800.0, 1000.0, 1200.0], groups),
                     rng.choice([150.0, 200.0, 250.0], groups), np.full(groups, 0.1),
                     np.round(rng.uniform(40, 120, groups), 2)], 1)
    write_xlsx(os.path.join(out, "Process_parameters.xlsx"), PROCESS_PARAMETERS, proc.tolist())


if __name__ == "__main__":
    main()
