"""Reference fixtures of the text-processing agents, ported:
TXT tests TextChunkerAgentTest.java:87-127, LanguageDetectorTest.java:37-39 and
TextExtractorTest.java (its two small PDF / DOCX documents are stored under
tests/golden/text_extractor/).

cl100k parity: no cl100k_base rank file exists offline, so the native BPE counter is a
synthetic-vocabulary byte-level BPE and its counts differ from tiktoken's ("parity
unpinned").  The cl100k fixture is therefore checked twice: the splitter's merge /
overlap algorithm with a counter that returns cl100k's real counts for the fixture's
words (must equal the reference output exactly), and the agent with the native counter
(chunk sizes within the configured budget)."""
import os

import pytest

from langstream_amd.agents.text import LanguageDetectorAgent, RecursiveCharacterTextSplitter, TextExtractorAgent, \
    TextSplitterAgent
from langstream_amd.api.record import SimpleRecord

RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_extractor")


def _chunks(cfg, text):
    a = TextSplitterAgent()
    a.init(cfg)
    return [r.value() for r in a.process_record(SimpleRecord.of("filename.txt", text.encode()))]


@pytest.mark.parametrize("size,overlap,text,expected", [
    (20, 5, "Hello world", ["Hello world"]),
    (15, 5, "Hello world. This is a great day", ["Hello world.", "This is a great", "great day"]),
    (20, 5, "", []),
    (20, 5, " ", []),
])
def test_chunker_length_fixtures(size, overlap, text, expected):
    cfg = {"splitter_type": "RecursiveCharacterTextSplitter", "separators": ["\n\n", "\n", " ", ""],
           "keep_separator": "false", "chunk_size": size, "chunk_overlap": overlap, "length_function": "length"}
    assert _chunks(cfg, text) == expected


def test_chunker_keep_separator_fixture():
    cfg = {"splitter_type": "RecursiveCharacterTextSplitter", "separators": ["\n\n", "\n", " ", ""],
           "keep_separator": True, "chunk_size": 15, "chunk_overlap": 5, "length_function": "length"}
    assert _chunks(cfg, "Hello world. This is a great day") == ["Hello world.", "This is a", "is a great day"]


# cl100k_base token counts of the fixture's pieces (one token each, "world," = world + ",")
_CL100K = {"Hello": 1, "world,": 2, "I": 1, "would": 1, "like": 1, "to": 1, "see": 1, "some": 1, "overlap": 1,
           "here": 1, " ": 1}


def _cl100k_like(s: str) -> int:
    if s in _CL100K:
        return _CL100K[s]
    return sum(_CL100K.get(w, 1) for w in s.split(" ")) + s.count(" ")


def test_chunker_cl100k_fixture_merge_algorithm():
    sp = RecursiveCharacterTextSplitter(["\n\n", "\n", " ", ""], False, 10, 2, _cl100k_like)
    assert sp.split_text("Hello world, I would like to see some overlap here") == \
        ["Hello world, I would like", "like to see some overlap", "overlap here"]
    sp = RecursiveCharacterTextSplitter(["\n\n", "\n", " ", ""], False, 20, 5, _cl100k_like)
    assert sp.split_text("Hello world") == ["Hello world"]


def test_chunker_cl100k_native_counter_budget():
    from langstream_amd.tokenizers import cl100k_counter
    count = cl100k_counter()
    cfg = {"chunk_size": 10, "chunk_overlap": 2, "length_function": "cl100k_base"}
    out = _chunks(cfg, "Hello world, I would like to see some overlap here")
    assert out and all(count(c) <= 10 for c in out)
    assert " ".join(out).replace("  ", " ").startswith("Hello world")


@pytest.mark.parametrize("text,lang", [("This is a English", "en"), ("Questo é italiano", "it"),
                                       ("Parlez-vous français?", "fr")])
def test_language_detector_fixtures(text, lang):
    a = LanguageDetectorAgent()
    a.init({"property": "detected-language"})
    out = a.process_record(SimpleRecord.of("filename.txt", text.encode()))
    assert out[0].header_value("detected-language") == lang


def test_language_detector_allowed_languages_filter():
    a = LanguageDetectorAgent()
    a.init({"property": "language", "allowedLanguages": ["en"]})
    assert a.process_record(SimpleRecord.of("k", "Questo é italiano")) == []
    assert len(a.process_record(SimpleRecord.of("k", "This is a English"))) == 1


def test_text_extractor_plain_text_fixture():
    a = TextExtractorAgent()
    out = a.process_record(SimpleRecord.of("filename.txt", b"This is a test"))
    assert out[0].value().strip() == "This is a test"


@pytest.mark.parametrize("fn,expected", [("simple.pdf", "This is a very simple PDF"),
                                         ("simple.docx", "This is a very simple Word Document")])
def test_text_extractor_binary_fixtures(fn, expected):
    with open(os.path.join(RES, fn), "rb") as f:
        data = f.read()
    out = TextExtractorAgent().process_record(SimpleRecord.of("filename", data))
    assert out[0].value().strip() == expected


def test_pdf_content_stream_text():
    """Flate-compressed content stream: literal-string escapes (\\( \\) octal), hex
    strings, TJ kerning (< -200/1000 em -> space), Td/T*/' line breaks."""
    import zlib
    from langstream_amd.agents.text import extract_text
    content = (b"BT /F1 12 Tf 72 712 Td (Hello \\(PDF\\) world) Tj 0 -14 Td [(Kern)-300(ed)20( text)] TJ "
               b"T* <48657820737472696E67> Tj\n(oct\\101l) ' ET")
    pdf = (b"%PDF-1.4\n1 0 obj << /Length 10 /Filter /FlateDecode >>\nstream\n" + zlib.compress(content)
           + b"\nendstream\nendobj\n%%EOF")
    assert extract_text(pdf) == "Hello (PDF) world\nKern ed text\nHex string\noctAl"


# Held-out sentences (food, technology, travel, sport, health): written for this test,
# none of them (nor the reference fixtures) appears in agents/langid_data.py.
HELD_OUT = {
    "da": ["Jeg har glemt min adgangskode til computeren igen.", "Toget til lufthavnen er desværre forsinket i dag.",
           "Hun løber fem kilometer hver tirsdag og torsdag.", "Lægen sagde, at jeg skal drikke mere vand.",
           "Vi spiste rugbrød med ost og en kop kaffe til frokost."],
    "de": ["Ich habe mein Passwort für den Computer schon wieder vergessen.",
           "Der Zug zum Flughafen hat heute leider Verspätung.", "Sie läuft jeden Dienstag fünf Kilometer.",
           "Der Arzt meinte, ich solle mehr Wasser trinken.", "Zum Mittagessen gab es Suppe mit frischem Gemüse."],
    "el": ["Ξέχασα πάλι τον κωδικό του υπολογιστή μου.", "Το τρένο για το αεροδρόμιο έχει καθυστέρηση σήμερα.",
           "Τρέχει πέντε χιλιόμετρα κάθε Τρίτη.", "Ο γιατρός είπε ότι πρέπει να πίνω περισσότερο νερό.",
           "Για μεσημεριανό φάγαμε σαλάτα με τυρί φέτα."],
    "en": ["I forgot the password for my laptop again.", "The train to the airport is delayed this morning.",
           "She runs five kilometres every Tuesday evening.", "The doctor told me to drink more water.",
           "We had soup and a sandwich for lunch."],
    "es": ["Otra vez he olvidado la contraseña del ordenador.", "El tren al aeropuerto llega tarde esta mañana.",
           "Ella corre cinco kilómetros todos los martes.", "El médico me dijo que bebiera más agua.",
           "Para almorzar tomamos una sopa de verduras y pan."],
    "et": ["Ma unustasin jälle oma arvuti parooli.", "Rong lennujaama hilineb täna hommikul.",
           "Ta jookseb igal teisipäeval viis kilomeetrit.", "Arst ütles, et ma pean rohkem vett jooma.",
           "Lõunaks sõime suppi ja musta leiba."],
    "fi": ["Unohdin taas tietokoneeni salasanan.", "Juna lentokentälle on tänään myöhässä.",
           "Hän juoksee viisi kilometriä joka tiistai.", "Lääkäri sanoi, että minun pitää juoda enemmän vettä.",
           "Söimme lounaaksi keittoa ja ruisleipää."],
    "fr": ["J'ai encore oublié le mot de passe de mon ordinateur.", "Le train pour l'aéroport a du retard ce matin.",
           "Elle court cinq kilomètres tous les mardis.", "Le médecin m'a dit de boire plus d'eau.",
           "Nous avons mangé une soupe et du fromage à midi."],
    "hu": ["Megint elfelejtettem a számítógépem jelszavát.", "A repülőtérre tartó vonat ma reggel késik.",
           "Minden kedden öt kilométert fut.", "Az orvos azt mondta, hogy több vizet kell innom.",
           "Ebédre levest és friss kenyeret ettünk."],
    "is": ["Ég gleymdi aftur lykilorðinu að tölvunni minni.", "Lestin út á flugvöll er sein í morgun.",
           "Hún hleypur fimm kílómetra á hverjum þriðjudegi.", "Læknirinn sagði að ég þyrfti að drekka meira vatn.",
           "Við borðuðum fiskisúpu og rúgbrauð í hádeginu."],
    "it": ["Ho dimenticato di nuovo la password del computer.", "Il treno per l'aeroporto è in ritardo stamattina.",
           "Lei corre cinque chilometri ogni martedì.", "Il medico mi ha detto di bere più acqua.",
           "A pranzo abbiamo mangiato una minestra di verdure."],
    "lt": ["Vėl pamiršau savo kompiuterio slaptažodį.", "Traukinys į oro uostą šį rytą vėluoja.",
           "Ji kiekvieną antradienį nubėga penkis kilometrus.", "Gydytojas pasakė, kad turiu gerti daugiau vandens.",
           "Pietums valgėme sriubą ir juodą duoną."],
    "nl": ["Ik ben het wachtwoord van mijn computer weer vergeten.", "De trein naar het vliegveld heeft vandaag vertraging.",
           "Ze loopt elke dinsdag vijf kilometer hard.", "De dokter zei dat ik meer water moet drinken.",
           "Als lunch aten we soep met een broodje kaas."],
    "no": ["Jeg har glemt passordet til datamaskinen min igjen.", "Toget til flyplassen er forsinket i dag.",
           "Hun løper fem kilometer hver tirsdag.", "Legen sa at jeg må drikke mer vann.",
           "Til lunsj spiste vi fiskesuppe og brødskiver med brunost."],
    "pl": ["Znowu zapomniałem hasła do komputera.", "Pociąg na lotnisko jest dziś rano opóźniony.",
           "Ona biega pięć kilometrów w każdy wtorek.", "Lekarz powiedział, że muszę pić więcej wody.",
           "Na obiad zjedliśmy zupę pomidorową i chleb."],
    "pt": ["Esqueci outra vez a palavra-passe do computador.", "O comboio para o aeroporto está atrasado hoje.",
           "Ela corre cinco quilómetros todas as terças-feiras.", "O médico disse que eu devia beber mais água.",
           "Ao almoço comemos uma sopa de legumes e pão."],
    "ru": ["Я опять забыл пароль от своего компьютера.", "Поезд в аэропорт сегодня утром опаздывает.",
           "Она бегает пять километров каждый вторник.", "Врач сказал, что мне нужно пить больше воды.",
           "На обед мы ели суп и чёрный хлеб."],
    "sv": ["Jag har glömt lösenordet till min dator igen.", "Tåget till flygplatsen är försenat i dag.",
           "Hon springer fem kilometer varje tisdag.", "Läkaren sa att jag måste dricka mer vatten.",
           "Till lunch åt vi ärtsoppa och pannkakor."],
    "th": ["ฉันลืมรหัสผ่านคอมพิวเตอร์อีกแล้ว", "รถไฟไปสนามบินมาสายในเช้านี้", "เธอวิ่งห้ากิโลเมตรทุกวันอังคาร",
           "หมอบอกว่าฉันควรดื่มน้ำให้มากขึ้น", "มื้อกลางวันเรากินข้าวผัดกับต้มยำกุ้ง"],
}


def test_language_detector_held_out_accuracy():
    """Generalisation over Tika's legacy profile set (LanguageDetectorAgent.java:55):
    >= 90 % of held-out sentences, none of which the profiles were built from."""
    from langstream_amd.agents.langid_data import SAMPLES
    from langstream_amd.agents.text import detect_language
    assert set(HELD_OUT) == set(SAMPLES) and len(SAMPLES) == 19
    corpus = " ".join(SAMPLES.values()).lower()
    wrong, total = [], 0
    for lang, sents in HELD_OUT.items():
        assert len(sents) >= 5
        for s in sents:
            assert s.lower().rstrip(".") not in corpus          # truly held out
            total += 1
            got = detect_language(s)
            if got != lang:
                wrong.append((lang, got, s))
    assert (total - len(wrong)) / total >= 0.90, wrong


def test_language_samples_do_not_contain_fixture_phrases():
    from langstream_amd.agents.langid_data import SAMPLES
    corpus = " ".join(SAMPLES.values()).lower()
    for phrase in ("this is a english", "questo é italiano", "parlez-vous français"):
        assert phrase not in corpus


def test_extractor_more_formats():
    """EPUB (spine order), gzip-wrapped, UTF-16 with BOM, generic XML, MIME e-mail."""
    import gzip
    import io
    import zipfile
    from langstream_amd.agents.text import extract_text
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        z.writestr("mimetype", "application/epub+zip")
        z.writestr("META-INF/container.xml",
                   '<container><rootfiles><rootfile full-path="OEBPS/content.opf"/></rootfiles></container>')
        z.writestr("OEBPS/content.opf",
                   '<package><manifest><item id="c2" href="ch2.xhtml"/><item id="c1" href="ch1.xhtml"/></manifest>'
                   '<spine><itemref idref="c1"/><itemref idref="c2"/></spine></package>')
        z.writestr("OEBPS/ch1.xhtml", "<html><body><p>Chapter one.</p></body></html>")
        z.writestr("OEBPS/ch2.xhtml", "<html><body><p>Chapter two.</p></body></html>")
    t = extract_text(buf.getvalue())
    assert t.index("Chapter one.") < t.index("Chapter two.")
    assert extract_text(gzip.compress("<html><body><p>zipped &amp; fine</p></body></html>".encode())) == "zipped & fine"
    assert extract_text("﻿hello world".encode("utf-16")) == "hello world"
    assert extract_text(b'<?xml version="1.0"?><note><to>Tove</to><msg>there &lt;3</msg></note>') == "Tove there <3"
    mail = ("From: a@example.com\nTo: b@example.com\nSubject: Quarterly report\nMIME-Version: 1.0\n"
            "Content-Type: multipart/alternative; boundary=XX\n\n--XX\nContent-Type: text/plain\n\n"
            "Numbers are up.\n--XX\nContent-Type: text/html\n\n<p>Numbers are <b>up</b>.</p>\n--XX--\n")
    assert extract_text(mail.encode()) == "Quarterly report\nNumbers are up."
