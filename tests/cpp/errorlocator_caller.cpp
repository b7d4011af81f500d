// A reference-style caller of PolarCode::Decoding::ErrorLocator through
// <polarcode/decoding/errorlocator.h>, as the reference's errorlocator tool uses it
// (src/errorlocator/simulator.cpp:185-193, 259-270): a reference decoder on the clean signal, its
// getOutput() as the desired output of the locating decoder on the noisy signal.
// "api": construction, accessors and argument errors, no GPU.
// "gpu <frozen.txt> <clean.bin> <noisy.bin> <F> <N>": the tool's flow per frame, then
// decodeFindFirstError, then the same frames through locateBatch, printed as hex for
// tests/test_gpu_errorlocator.py.
#include <polarcode/decoding/errorlocator.h>

#include <cstdio>
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

static std::vector<float> floats(const char* path, size_t n)
{
    std::vector<float> v(n);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float)));
    return v;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "api";
    if (mode == "api") {
        std::vector<unsigned> fr;
        for (unsigned i = 0; i < 512; ++i)
            fr.push_back(i);
        Decoding::ErrorLocator* el = new Decoding::ErrorLocator(1024, fr);
        Decoding::Decoder* dec = el; // the reference's virtual interface
        if (dec->blockLength() != 1024 || dec->infoLength() != 512 || dec->getListSize() != 1)
            return 1;
        if (el->firstError() != -1 || el->correctionCount() != 0 || el->getOutput().size() != 1024)
            return 2;
        el->setAsReferenceDecoder();
        el->setDesiredOutput(std::vector<float>(1024, -1.0f));
        el->initialize(1024, fr); // the same code: nothing happens
        el->initialize(64, { 0, 1, 2, 4, 8 });
        if (dec->blockLength() != 64 || dec->infoLength() != 59 || el->getOutput().size() != 64)
            return 3;
        el->clear();
        int refused = 0;
        try {
            el->setDesiredOutput(std::vector<float>(63, 0.0f)); // too short
        } catch (const std::logic_error&) {
            ++refused;
        }
        delete el;
        try {
            Decoding::ErrorLocator bad(24, { 0 }); // not a power of two
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::ErrorLocator bad(8, { 0, 1, 2, 3, 4, 5, 6, 7 }); // no information bit
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::ErrorLocator bad(16, { 3, 2 }); // not ascending
        } catch (const std::logic_error&) {
            ++refused;
        }
        try {
            Decoding::ErrorLocator bad(8192, { 0 }); // above the kernel's block-length limit
        } catch (const std::runtime_error&) {
            ++refused;
        }
        if (refused != 5)
            return 4;
        std::printf("errorlocator api ok\n");
        return 0;
    }
    if (mode == "gpu" && argc >= 7) {
        std::vector<unsigned> fr;
        std::ifstream ff(argv[2]);
        for (unsigned v; ff >> v;)
            fr.push_back(v);
        const size_t F = std::stoul(argv[5]), N = std::stoul(argv[6]);
        const std::vector<float> clean = floats(argv[3], F * N), noisy = floats(argv[4], F * N);
        Decoding::ErrorLocator decoder(N, fr), reference(N, fr);
        reference.setAsReferenceDecoder();
        std::vector<float> words(N), desired(F * N);
        for (size_t f = 0; f < F; ++f) {
            reference.setSignal(clean.data() + f * N);
            reference.decode();
            decoder.setSignal(noisy.data() + f * N);
            decoder.setDesiredOutput(reference.getOutput());
            const bool r = decoder.decode();
            const std::vector<float> out = decoder.getOutput();
            decoder.getSoftCodeword(words.data());
            std::printf("%d %d %d ", r ? 1 : 0, decoder.firstError(), decoder.correctionCount());
            hex(out.data(), N * sizeof(float));
            std::printf(" ");
            hex(words.data(), N * sizeof(float));
            std::printf(" %d\n", decoder.decodeFindFirstError());
            const std::vector<float> ro = reference.getOutput();
            for (size_t i = 0; i < N; ++i)
                desired[f * N + i] = ro[i];
        }
        std::vector<float> u(F * N);
        std::vector<uint32_t> bits(F * N), count(F);
        std::vector<int32_t> first(F);
        decoder.locateBatch(Decoding::ErrorLocator::Correct, noisy.data(), desired.data(), F, u.data(), bits.data(),
                            first.data(), count.data());
        hex(u.data(), u.size() * sizeof(float));
        std::printf(" ");
        hex(bits.data(), bits.size() * sizeof(uint32_t));
        std::printf(" ");
        hex(first.data(), F * sizeof(int32_t));
        std::printf(" ");
        hex(count.data(), F * sizeof(uint32_t));
        std::printf("\nerrorlocator gpu ok\n");
        return 0;
    }
    return 64;
}
