// A reference-style caller of PolarCode::Decoding::DepthFirst through
// <polarcode/decoding/depth_first.h> (new Decoding::DepthFirst(N, trialLimit, frozen), as
// simulator.cpp:715-716 constructs it).
// "api": construction, accessors and argument errors, no GPU.
// "gpu <frozen.txt> <llr.bin> <F> <N> <trial limit> <systematic>": setSignal -> decode ->
// getDecodedInformationBits -> getSoftCodeword per frame, then the same frames through
// decodeBatch, printed as hex for tests/test_gpu_depthfirst.py.
#include <polarcode/decoding/depth_first.h>
#include <polarcode/errordetection/crc8.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace PolarCode;

static void hex(const void* p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        std::printf("%02x", static_cast<const unsigned char*>(p)[i]);
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "api";
    if (mode == "api") {
        std::vector<unsigned> fr;
        for (unsigned i = 0; i < 512; ++i)
            fr.push_back(i);
        Decoding::DepthFirst* df = new Decoding::DepthFirst(1024, 8, fr);
        Decoding::Decoder* dec = df; // the reference's virtual interface
        if (dec->blockLength() != 1024 || dec->infoLength() != 512 || dec->getListSize() != 8 || !dec->isSystematic())
            return 1;
        df->setTrialLimit(2);
        if (dec->getListSize() != 2 || df->trials() != 0)
            return 2;
        ErrorDetection::CRC8 crc;
        dec->setErrorDetection(&crc);
        if (dec->getErrorDetectionMode() != "CRC-8")
            return 3;
        dec->setSystematic(false);
        if (dec->isSystematic())
            return 3;
        df->initialize(64, 3, { 0, 1, 2, 4, 8 });
        if (dec->blockLength() != 64 || dec->infoLength() != 59 || dec->getListSize() != 3)
            return 4;
        int refused = 0;
        try {
            df->setTrialLimit(0);
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            df->setTrialLimit(60); // more trials than information bits
        } catch (const std::logic_error&) {
            ++refused;
        }
        delete df;
        try {
            Decoding::DepthFirst bad(24, 1, { 0 }); // not a power of two
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::DepthFirst bad(64, 0, { 0 }); // no trials
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            // one information bit: the reference reads past its list
            Decoding::DepthFirst bad(8, 1, { 0, 1, 2, 3, 4, 5, 6 });
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::DepthFirst bad(8192, 1, { 0 }); // above the kernel's block-length limit
        } catch (const std::runtime_error&) {
            ++refused;
        }
        if (refused != 6)
            return 5;
        std::printf("depthfirst api ok\n");
        return 0;
    }
    if (mode == "gpu" && argc >= 8) {
        std::vector<unsigned> fr;
        std::ifstream ff(argv[2]);
        for (unsigned v; ff >> v;)
            fr.push_back(v);
        const size_t F = std::stoul(argv[4]), N = std::stoul(argv[5]);
        std::vector<float> llr(F * N);
        std::ifstream lf(argv[3], std::ios::binary);
        lf.read(reinterpret_cast<char*>(llr.data()), (std::streamsize)(llr.size() * sizeof(float)));
        Decoding::DepthFirst dec(N, std::stoul(argv[6]), fr);
        ErrorDetection::CRC8 crc;
        dec.setErrorDetection(&crc);
        dec.setSystematic(std::stoul(argv[7]) != 0);
        const size_t kb = (dec.infoLength() + 7) / 8;
        std::vector<float> words(N);
        std::vector<unsigned char> info(kb);
        for (size_t f = 0; f < F; ++f) {
            dec.setSignal(llr.data() + f * N);
            const bool ok = dec.decode();
            dec.getSoftCodeword(words.data());
            dec.getDecodedInformationBits(info.data());
            std::printf("%d %u ", ok ? 1 : 0, dec.trials());
            hex(info.data(), info.size());
            std::printf(" ");
            hex(words.data(), N * sizeof(float));
            std::printf("\n");
        }
        std::vector<unsigned char> binfo(F * kb), bok(F), btr(F);
        std::vector<uint32_t> bbits(F * N);
        dec.decodeBatchBits(llr.data(), F, binfo.data(), bok.data(), bbits.data(), btr.data());
        hex(binfo.data(), binfo.size());
        std::printf(" ");
        hex(bok.data(), F);
        std::printf(" ");
        hex(btr.data(), F);
        std::printf(" ");
        hex(bbits.data(), bbits.size() * sizeof(uint32_t));
        std::printf("\ndepthfirst gpu ok\n");
        return 0;
    }
    return 64;
}
