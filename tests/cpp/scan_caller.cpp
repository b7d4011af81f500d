// A reference-style caller of PolarCode::Decoding::Scan through <polarcode/decoding/scan.h>
// (decodingtest.cpp:1230-1256 constructs it the same way).  "api": construction, accessors and
// argument errors, no GPU.  "gpu <frozen.txt> <llr.bin> <F> <iterations>": setSignal -> decode ->
// getSoftCodeword / getExtrinsicChannelInformation / getDecodedInformationBits per frame, printed
// as hex for tests/test_gpu_scan.py.
#include <polarcode/decoding/scan.h>
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
        Decoding::Scan* scan = new Decoding::Scan(1024, 4, fr);
        Decoding::Decoder* dec = scan; // the reference's virtual interface
        if (dec->blockLength() != 1024 || dec->infoLength() != 512 || dec->getListSize() != 4 || !dec->isSystematic())
            return 1;
        scan->setIterationLimit(2);
        if (dec->getListSize() != 2)
            return 2;
        ErrorDetection::CRC8 crc;
        dec->setErrorDetection(&crc);
        if (dec->getErrorDetectionMode() != "CRC-8")
            return 3;
        scan->initialize(64, 3, { 0, 1, 2, 4, 8 });
        if (dec->blockLength() != 64 || dec->infoLength() != 59 || dec->getListSize() != 3)
            return 4;
        delete scan;
        int refused = 0;
        try {
            Decoding::Scan bad(24, 1, { 0 }); // not a power of two
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::Scan bad(64, 256, { 0 }); // more than 255 iterations
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::Scan bad(8192, 1, { 0 }); // above the kernel's block-length limit
        } catch (const std::runtime_error&) {
            ++refused;
        }
        if (refused != 3)
            return 5;
        std::printf("scan api ok\n");
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
        Decoding::Scan dec(N, (unsigned)std::stoul(argv[5]), fr);
        ErrorDetection::CRC8 crc;
        dec.setErrorDetection(&crc);
        const size_t K = dec.infoLength();
        std::vector<float> soft(N), ext(N), sinfo(K);
        std::vector<unsigned char> info((K + 7) / 8);
        for (size_t f = 0; f < F; ++f) {
            dec.setSignal(llr.data() + f * N);
            const bool ok = dec.decode();
            dec.getSoftCodeword(soft.data());
            dec.getSoftInformation(sinfo.data());
            dec.getExtrinsicChannelInformation(ext.data());
            dec.getDecodedInformationBits(info.data());
            std::printf("%d ", ok ? 1 : 0);
            hex(info.data(), info.size());
            std::printf(" ");
            hex(soft.data(), N * sizeof(float));
            std::printf(" ");
            hex(ext.data(), N * sizeof(float));
            std::printf(" ");
            hex(sinfo.data(), K * sizeof(float));
            std::printf("\n");
        }
        std::printf("scan gpu ok\n");
        return 0;
    }
    return 64;
}
