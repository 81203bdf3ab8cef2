! The actinic flux through the Fortran shell: specifyParameters(computeActinicFlux = .true.) and reportResults(actinicFlux =) on a
! small cloud over a reflecting surface, irregular layers.  Prints, per layer, the field of every column
! (tests/test_gpu_actinic_flux.py runs the same photons through the Python mirror), and what the shell answers when the field is
! asked for without having been computed, or into an array of the wrong shape.
program actinicFluxTest
  use ErrorMessages
  use RandomNumbers
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloIllumination
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 50000
  type(ErrorMessage)         :: status
  type(domain)               :: cloud
  type(integrator)           :: mc
  type(randomNumberSequence) :: randoms
  type(photonStream)         :: photons
  type(phaseFunction)        :: hg
  type(phaseFunctionTable)   :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), field(nx, ny, nz), wrong(nx, ny, nz + 1)
  integer :: idx(nx, ny, nz), i, j, k

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, status = status)

  ! asked for before it is switched on
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  call finalize_PhotonStream(photons)
  call initializeState(status)
  call reportResults(mc, status = status, actinicFlux = field)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  call specifyParameters(mc, status = status, computeActinicFlux = .true.)
  if(stateIsFailure(status)) then
    print *, "specifyParameters(computeActinicFlux) failed"; stop 1
  end if
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransfer failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportResults(mc, status = status, actinicFlux = wrong)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportResults(mc, status = status, actinicFlux = field)
  if(stateIsFailure(status)) then
    print *, "reportResults failed: ", trim(failureText()); stop 1
  end if
  do k = 1, nz
    print '(a, i3, 8f10.6)', "actinic   ", k - 1, ((field(i, j, k), i = 1, nx), j = 1, ny)
  end do
  ! switched off again: the array is gone
  call specifyParameters(mc, status = status, computeActinicFlux = .false.)
  call initializeState(status)
  call reportResults(mc, status = status, actinicFlux = field)
  print '(a, l2)', "offagain    ", stateIsFailure(status)
  call finalize_Integrator(mc)
  print '(a)', "actinicFluxTest done"
contains
  ! the oldest message of the status object (the probes start from a fresh one)
  function failureText() result(text)
    character(len = 256) :: text
    call firstMessage(status)
    text = getCurrentMessage(status)
  end function failureText
end program actinicFluxTest
