// A reference-style caller of PolarCode::Decoding::FastSscanFloat through
// <polarcode/decoding/fastsscan_float.h> (decodingtest.cpp:1259-1272 constructs it the same way).
// "api": construction, accessors and argument errors, no GPU.
// "gpu <frozen.txt> <llr.bin> <F> <trial limit>": setSignal -> decode -> getSoftCodeword ->
// decodeAgain -> getSoftCodeword per frame, printed as hex for tests/test_gpu_fsscan.py.
#include <polarcode/decoding/fastsscan_float.h>
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
        Decoding::FastSscanFloat* fss = new Decoding::FastSscanFloat(1024, 4, fr);
        Decoding::Decoder* dec = fss; // the reference's virtual interface
        if (dec->blockLength() != 1024 || dec->infoLength() != 512 || dec->getListSize() != 4 || !dec->isSystematic())
            return 1;
        fss->setTrialLimit(2);
        if (dec->getListSize() != 2 || fss->trials() != 0)
            return 2;
        ErrorDetection::CRC8 crc;
        dec->setErrorDetection(&crc);
        if (dec->getErrorDetectionMode() != "CRC-8")
            return 3;
        fss->initialize(64, 3, { 0, 1, 2, 4, 8 });
        if (dec->blockLength() != 64 || dec->infoLength() != 59 || dec->getListSize() != 3)
            return 4;
        int refused = 0;
        try {
            fss->decodeAgain(); // nothing decoded yet
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            fss->setTrialLimit(0);
        } catch (const std::logic_error&) {
            ++refused;
        }
        delete fss;
        try {
            Decoding::FastSscanFloat bad(24, 1, { 0 }); // not a power of two
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::FastSscanFloat bad(64, 0, { 0 }); // no passes
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::FastSscanFloat bad(8192, 1, { 0 }); // above the kernel's block-length limit
        } catch (const std::runtime_error&) {
            ++refused;
        }
        if (refused != 5)
            return 5;
        std::printf("fsscan api ok\n");
        return 0;
    }
    if (mode == "gpu" && argc >= 6) {
        std::vector<unsigned> fr;
        std::ifstream ff(argv[2]);
        for (unsigned v; ff >> v;)
            fr.push_back(v);
        const size_t F = std::stoul(argv[4]), N = 1024;
        std::vector<float> llr(F * N);
        std::ifstream lf(argv[3], std::ios::binary);
        lf.read(reinterpret_cast<char*>(llr.data()), (std::streamsize)(llr.size() * sizeof(float)));
        Decoding::FastSscanFloat dec(N, (unsigned)std::stoul(argv[5]), fr);
        ErrorDetection::CRC8 crc;
        dec.setErrorDetection(&crc);
        const size_t K = dec.infoLength();
        std::vector<float> soft(N), again(N), sinfo(K);
        std::vector<unsigned char> info((K + 7) / 8), info2((K + 7) / 8);
        for (size_t f = 0; f < F; ++f) {
            dec.setSignal(llr.data() + f * N);
            const bool ok = dec.decode();
            const unsigned t = dec.trials();
            dec.getSoftCodeword(soft.data());
            dec.getSoftInformation(sinfo.data());
            dec.getDecodedInformationBits(info.data());
            const bool ok2 = dec.decodeAgain();
            if (dec.trials() != t + 1)
                return 6;
            dec.getSoftCodeword(again.data());
            dec.getDecodedInformationBits(info2.data());
            std::printf("%d %u ", ok ? 1 : 0, t);
            hex(info.data(), info.size());
            std::printf(" ");
            hex(soft.data(), N * sizeof(float));
            std::printf(" ");
            hex(sinfo.data(), K * sizeof(float));
            std::printf(" %d ", ok2 ? 1 : 0);
            hex(info2.data(), info2.size());
            std::printf(" ");
            hex(again.data(), N * sizeof(float));
            std::printf("\n");
        }
        std::printf("fsscan gpu ok\n");
        return 0;
    }
    return 64;
}
