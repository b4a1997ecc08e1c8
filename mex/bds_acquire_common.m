function acqResults = bds_acquire_common(longSignal, settings, signal)
% Shared body of the drop-in acquisition wrappers: converts the MATLAB arguments,
% calls the MEX gateway (bds_mex -> libbds_mi355x.so) and prints the reference's
% "(19 20 . )" line (acquisition.m:167,259,360,366).
%   signal: 1 = B1C, 2 = B2a
if settings.fileType == 3
    % packed record: uint8 bytes as fread(fid, n/2, 'uint8=>uint8') returns them, two 2+2-bit I/Q samples each
    % (B2a/include/unpack_cplx.m:18-30); they go to the library as they are
    if ~isa(longSignal, 'uint8')
        error('bds:arg', 'longSignal must be uint8 packed bytes when settings.fileType is 3');
    end
    [carrFreq, codePhase, peakMetric, detected] = bds_mex('acquire', longSignal(:).', settings, signal, 2);
    iq = 2;
else
    iq = ~isreal(longSignal);
end
if iq == 1
    % fileType 2: longSignal = data(1:2:end) + 1i*data(2:2:end) (postProcessing.m:92-96);
    % hand the int8 pairs back interleaved
    pairs = [real(longSignal(:)).'; imag(longSignal(:)).'];
    longSignal = pairs(:).';
end
if iq ~= 2
    if any(longSignal ~= round(longSignal)) || any(longSignal > 127) || any(longSignal < -128)
        error('bds:arg', 'longSignal must hold int8 values (fread(...,''schar''))');
    end
    [carrFreq, codePhase, peakMetric, detected] = bds_mex('acquire', int8(longSignal), settings, signal, iq);
end
acqResults.carrFreq   = carrFreq;
acqResults.codePhase  = codePhase;
acqResults.peakMetric = peakMetric;
fprintf('(');
for PRN = settings.acqSatelliteList
    if detected(PRN), fprintf('%02d ', PRN); else, fprintf('. '); end
end
fprintf(')\n');
end
