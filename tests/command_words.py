"""A micro model file whose vocabulary holds a few real words, for the text form of command lists: the synthetic files spell
token t " w<t>", which ohw_tokenize cuts into a letter piece and a digit piece and so never finds."""
from openhush_amd import modelfile

WORDS = {47018: b" lights", 47019: b"lights", 17019: b" on", 17020: b"on", 20198: b" off", 20199: b"off"}
PHRASES = ["lights", "on off", "off lights"]
# what ohw_tokenize makes of each text as given and with a leading space, and the text's index
FORMS = [[47019], [47018], [17020, 20198], [17019, 20198], [20199, 47018], [20198, 47018]]
INDEX = [0, 0, 1, 1, 2, 2]


def worded_model(src: str, dst: str) -> str:
    """src's tensors under a vocabulary with WORDS in it, written to dst"""
    hp, filt, vocab, raw = modelfile.read_model_raw(src)
    for t, w in WORDS.items():
        vocab[t] = w
    modelfile.write_model(dst, hp.as_list(), filt, vocab, raw)
    return dst
